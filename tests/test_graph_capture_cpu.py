"""The table of tests/graph_capture.py held to include/srhip.h, without a GPU and without HIP: every prototype that takes a `void* stream`
has a capture row or a reason why it is not captured, so that an entry point cannot be added without its row in
tests/test_gpu_graph_capture.py."""
import os

import graph_capture as gc
import stream_order as so


def test_the_table_module_needs_no_gpu():
    assert gc.ROWS and "torch" not in vars(gc) and "rusty_sr_amd" not in vars(gc)
    assert all(hasattr(so.Builders, row["build"]) for row in gc.ROWS)


def test_every_stream_prototype_has_a_capture_row_or_a_reason():
    protos = so.stream_prototypes()
    assert len(protos) >= 42
    rows = {row["entry"] for row in gc.ROWS}
    by_id = {row["id"]: row for row in so.ROWS}
    assert all(i in by_id and reason.strip() for i, reason in gc.NOT_CAPTURED.items())
    excused = {by_id[i]["entry"] for i in gc.NOT_CAPTURED}
    assert set(protos) - rows - excused == set(), "entry points of include/srhip.h with neither a capture row nor a reason"
    assert rows - set(protos) == set(), "rows that name no prototype of include/srhip.h"
    assert set(protos) - rows == set(), "today every entry point is captured on a side stream: only the NULL-stream rows are excused"


def test_a_new_prototype_without_a_row_is_seen():
    header = "int sr_new_thing_dev(sr_ctx* ctx, const float* d_in, float* d_out, void* stream);"
    assert set(so.stream_prototypes(header)) - {row["entry"] for row in gc.ROWS} == {"sr_new_thing_dev"}


def test_coverage_rules_of_the_table():
    ids = [row["id"] for row in gc.ROWS]
    assert len(ids) == len(set(ids)) and not set(ids) & set(gc.NOT_CAPTURED)
    have = {(r["entry"], r["precision"], r["factor"], r["fork"]) for r in gc.ROWS}
    assert all(r["stream"] == "side" for r in gc.ROWS)
    for entry in so.NETWORK:   # network calls: both precisions at factor 3
        for precision in ("f32", "split_f16"):
            assert (entry, precision, 3, None) in have, (entry, precision)
    for entry in so.OTHER:
        assert (entry, "f32", 3, None) in have, entry
    plain = "sr_upscale_rgba8_dev"
    assert {(plain, "f32", 2, None), (plain, "f32", 4, None)} <= have
    for cut in so.FORKS:       # a captured fork replays as two parallel branches of the graph
        assert (plain, "f32", 3, cut) in have and (plain, "split_f16", 3, cut) in have
    # the three NULL-stream rows of the stream-order table, and nothing else
    assert sorted(gc.NOT_CAPTURED) == sorted(r["id"] for r in so.ROWS if r["stream"] == "null") and len(gc.NOT_CAPTURED) == 3


def test_the_header_states_the_contract():
    text = open(os.path.join(so.ROOT, "include", "srhip.h")).read()
    assert "Stream capture" in text
    block = text[text.index("Stream capture"):]
    block = block[:block.index("*/")]
    for k in range(1, 9):      # its eight points
        assert f" {k}. " in block, k
    for word in ("SR_E_INVALID", "UNDEFINED", "sr_set_params", "sr_set_precision", "srhip_experimental.h", "sr_set_loss", "sr_reserve_",
                 "stream = NULL", "sr_check_domain", "fork tuner"):
        assert word in block, word
    # (include/srhip.h names no experiment switch, tests/test_abi.py: the setter's own header says what it does to a graph)
    assert "Stream capture" in open(os.path.join(so.ROOT, "include", "srhip_experimental.h")).read()
