// border_index.cpp -- sr_border.h's index rule driven from a plain C++ program (tests/test_border_cpu.py): the header the pad kernel
// compiles is compiled here by g++ alone, and its answers are printed for numpy to compare with np.pad.
//
//   border_index MODE SIZE PAD   prints sr_border_index(j - PAD, SIZE, MODE) for j = 0 .. SIZE + 2 PAD - 1, one line, space separated
//
// Several triples may follow one another; each prints its own line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rusty_sr_amd/csrc/sr_border.h"

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: border_index MODE SIZE PAD [MODE SIZE PAD ...]\n");
        return 2;
    }
    for (int k = 1; k + 2 < argc; k += 3) {
        const int mode = atoi(argv[k]), size = atoi(argv[k + 1]), pad = atoi(argv[k + 2]);
        if (mode < 1 || mode > 3 || size < 1 || pad < 0) {
            fprintf(stderr, "bad triple %s %s %s\n", argv[k], argv[k + 1], argv[k + 2]);
            return 2;
        }
        std::vector<int> idx((size_t)size + 2 * (size_t)pad);
        for (int j = 0; j < size + 2 * pad; ++j) idx[(size_t)j] = sr_border_index(j - pad, size, mode);
        for (size_t j = 0; j < idx.size(); ++j) {
            if (idx[j] < 0 || idx[j] >= size) {
                fprintf(stderr, "index %d out of range at %zu\n", idx[j], j);
                return 1;
            }
            printf(j ? " %d" : "%d", idx[j]);
        }
        printf("\n");
    }
    return 0;
}
