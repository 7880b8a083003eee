// sr_border.h -- the index rule of the border modes (include/srhip.h "Borders"): which sample of an axis of `size` samples stands at
// position i of its continuation, for ANY integer i.  Shared by border_pad_kernel (sr_border.hip) and the host (tests/c/border_index.cpp
// compiles it with a plain C++ compiler and holds it to numpy's np.pad).  Plain integer arithmetic, no HIP.
#pragma once

#if defined(__HIPCC__)
#define SR_BORDER_FN __host__ __device__ __forceinline__
#else
#define SR_BORDER_FN inline
#endif

// modes: include/srhip.h SR_BORDER_WRAP 1, SR_BORDER_REPLICATE 2, SR_BORDER_MIRROR 3.  size >= 1 and 2 size <= INT_MAX.
//   wrap       i mod size, a true modulo: a size below the pad goes round more than once
//   replicate  i clamped to [0, size - 1]
//   mirror     a reflection that repeats the edge sample (... 1 0 | 0 1 2 | 2 1 ...), of period 2 size
SR_BORDER_FN int sr_border_index(int i, int size, int mode) {
    if (i >= 0 && i < size) return i;
    if (mode == 2) return i < 0 ? 0 : size - 1;
    const int period = mode == 1 ? size : 2 * size;
    int m = i % period;
    if (m < 0) m += period;
    return m < size ? m : 2 * size - 1 - m;
}
