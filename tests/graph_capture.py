"""The stream-capture contract of the *_dev entry points (include/srhip.h "Stream capture") as a table and one helper.

ROWS is tests/stream_order.py's table on its first caller's stream: one row for every prototype of include/srhip.h that takes a
`void* stream`, in both arithmetic modes where the result depends on the mode, the two forced-fork plans of sr_upscale_rgba8_dev and
factors 2 and 4.  The rows of that table on stream = NULL are NOT_CAPTURED, each with its reason.  tests/test_graph_capture_cpu.py holds
the table to the header without a GPU, so nothing at module level here needs torch, HIP or the library; tests/test_gpu_graph_capture.py
runs it.

replayed() is the test of one row.  ONE call is captured into a graph (torch.cuda.graph on a side stream, torch's default error mode)
on tensors that exist beforehand, and replayed:

    eager decoy, eager real | capture on decoy | sync | real, replay | decoy, replay | decoy, replay, replay | eager real | decoy, replay

What is asserted, and what it answers for:
  status    the captured call returns SR_OK (a warm call has nothing to allocate)
  capture   after the capture the outputs still hold the first sentinel: capturing ran nothing
  replay    the replay on `real` is the eager result on `real`: every launch of the call was recorded, on whatever stream it runs
  unbaked   the replay on `decoy`, over a second sentinel, is the eager result on `decoy`: nothing but pointers was recorded
  twice     two replays with no synchronisation between them still give it: a replay leaves nothing behind that the next one trips over
  mixed     an eager call of the same shape between two replays gets its result, and so does the replay after it
Every comparison is on bytes.  The reference is the same call made eagerly (which the other GPU tests hold to the oracle).  No graph is
ever replayed after anything that could grow or free what it points to: every shape a test uses runs eagerly before the first capture."""
import stream_order as so

LEGS = ("status", "capture", "replay", "unbaked", "twice", "mixed")

NULL_REASON = ("stream = NULL is HIP's legacy stream: it cannot be captured, and the library cannot see a capture it takes part in "
               "(include/srhip.h \"Stream capture\", point 6)")
NOT_CAPTURED = {row["id"]: NULL_REASON for row in so.ROWS if row["stream"] == "null"}
ROWS = [dict(row) for row in so.ROWS if row["stream"] == "side"]


def diff_report(got, want):
    """Where two tensors of one shape differ, in words: how many bytes, and for an image (n, H, W, C) which rows and columns."""
    import torch
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    nbytes = int((so._bytes(got) != so._bytes(want)).sum())
    if nbytes == 0:
        return "equal"
    text = f"{nbytes} of {so._bytes(got).numel()} bytes differ"
    if got.dim() == 4:
        px = (got.view(torch.uint8).reshape(got.shape[0], got.shape[1], got.shape[2], -1)
              != want.view(torch.uint8).reshape(got.shape[0], got.shape[1], got.shape[2], -1)).any(dim=-1).any(dim=0)
        rows = torch.nonzero(px.any(dim=1)).flatten().tolist()
        cols = torch.nonzero(px.any(dim=0)).flatten().tolist()
        text += (f"; {int(px.sum())} pixels in rows {rows[0]}..{rows[-1]} ({len(rows)} of {got.shape[1]}) and columns {cols[0]}..{cols[-1]} "
                 f"({len(cols)} of {got.shape[2]})")
    return text


def differs(got, want):
    """None where every tensor of `got` is `want`'s bytes, else diff_report of the first that is not."""
    for k, (a, b) in enumerate(zip(got, want)):
        if not so.same(a, b):
            return f"tensor {k}: {diff_report(a, b)}"
    return None


def capture(case, stream):
    """The graph of ONE call of `case` on the tensors it holds, captured on `stream` under torch's default error mode ("global": what a
    PyTorch caller gets).  The call raises whatever status it returns; the capture is ended either way."""
    import torch
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        case.run(stream)
    return g


def replay(case, g, stream, src, sentinel=so.SENTINELS[1], times=1):
    """inputs <- src, outputs <- sentinel, `times` replays on `stream` with no host synchronisation between them (a call that writes
    into its inputs gets them back, queued, before each), then a synchronisation; -> a snapshot of what the call writes."""
    import torch
    with torch.cuda.stream(stream):
        case.fill_outs(sentinel)
        for _ in range(times):
            case.load(src)
            g.replay()
    torch.cuda.synchronize()
    return so.snapshot(case.written)


def eager(case, stream, src, sentinel=so.SENTINELS[0]):
    """the same call made eagerly and synchronously on `src`; -> a snapshot of what it writes"""
    import torch
    with torch.cuda.stream(stream):
        case.load(src)
        case.fill_outs(sentinel)
        case.run(stream)
    torch.cuda.synchronize()
    return so.snapshot(case.written)


def replayed(case, stream, check_after=None, name=""):
    """One row (the module's text).  check_after(): what else must hold at the end.  Returns the legs that ran; raises AssertionError
    with every leg that failed."""
    import torch
    failed = []
    want, want_decoy, _ = so.reference(case, stream)                                    # 1 (warm: code, tables, workspace)
    with torch.cuda.stream(stream):                                                     # 2
        case.load(case.decoy)
        case.fill_outs(so.SENTINELS[0])
    torch.cuda.synchronize()
    before = so.snapshot(case.written)   # the first sentinel; a tensor the call writes in place holds its decoy
    g = capture(case, stream)            # (a status other than SR_OK raises)
    try:
        torch.cuda.synchronize()                                                        # 3
        d = differs(case.written, before)
        if d:
            failed.append(f"capture: the captured call wrote ({d})")
        d = differs(replay(case, g, stream, case.real), want)                           # 4
        if d:
            failed.append(f"replay: on the real input, not the eager result ({d})")
        d = differs(replay(case, g, stream, case.decoy), want_decoy)                    # 5
        if d:
            failed.append(f"unbaked: on the decoy, not the eager result ({d})")
        d = differs(replay(case, g, stream, case.decoy, so.SENTINELS[0], times=2), want_decoy)   # 6
        if d:
            failed.append(f"twice: two replays back to back ({d})")
        d = differs(eager(case, stream, case.real), want)                               # 7
        if d:
            failed.append(f"mixed: the eager call between two replays ({d})")
        d = differs(replay(case, g, stream, case.decoy), want_decoy)
        if d:
            failed.append(f"mixed: the replay after an eager call ({d})")
        if check_after is not None:
            check_after()
    finally:
        del g
        torch.cuda.synchronize()
    assert not failed, f"{name}: " + "; ".join(failed)
    return list(LEGS)
