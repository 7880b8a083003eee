"""The tile-queue case table: calls planned for 1-5 compute units (sr_set_experiment "cus"), at which the persistent pipe form of the stage
kernels (sr_kernels.hip conv_stage_pipe_kernel) runs its per-XCD tile queues, its steals and its change of tile class on images small
enough for the oracle and its node taps -- and a numpy restatement of the queue's index arithmetic.

A case is a case of tests/plan_cases.py (the same words, so plan_cases.check_line / run_plan_check plan it) plus
    cus    the compute units the call is planned for
    ch     bytes per input pixel of a u8 call (4: RGBA with a random alpha plane)
    reach  what the case is in the table for -- tests/test_tile_queue_cpu.py holds every claim to the HIP-free planner's lines:
        queue         a pipe launch with fewer workgroups than tiles: tiles come from the queue
        mixed         8-row and 4-row tiles in one pipe launch: a workgroup changes tile class in mid-launch
        ownerless     a pipe launch of fewer than 8 workgroups and more non-empty XCD runs than workgroups: whole queues that only steals empty
        deep          a pipe launch of 16 or more tiles per workgroup
        fork          the call runs as two bands (exact f32: by the automatic rule unless the case sets "fork"; the split-half mode never
                      forks by the rule, there the switch does it)
        conv0-rounds  conv0 has more tiles than its 8 workgroups per compute unit: its stride loop goes round
        control       no launch asks the queue: first form, or a pipe launch with a workgroup per tile
    host   a host-pointer call's chunk plan, "inorder" | "alternating" (its bands are set with "rows": the host-chunk planner cuts by
           pixels and bytes, not by compute units, and leaves an image this small whole)
    oracle whether the GPU test also holds the case to the oracle (shapes up to 61 x 97; larger ones: plan, bit identity, repeatability)"""
import itertools

PROPERTIES = ("queue", "mixed", "ownerless", "deep", "fork", "conv0-rounds", "control")
PRECISIONS = ("f32", "split_f16")
FIVE = "84848"  # a five-digit "th": 8-row tiles in stages 0, 2, 4, 4-row tiles in stages 1 and 3


# ---- the queue's index arithmetic (sr_kernels.hip run_of_xcd, queue_slot, queue_total, queue_first; conv0's head preset) ----
def run_of_xcd(x, ntiles):
    """-> (start, count) of XCD x's contiguous run of a class of ntiles tiles"""
    q, r = ntiles >> 3, ntiles & 7
    return (x * (q + 1), q + 1) if x < r else (r * (q + 1) + (x - r) * q, q)


def queue_slot(x, nbig, nsmall, idx):
    """entry idx of XCD x's queue -- its run of big tiles, then its run of small ones -- as a combined tile id; -1 past its end"""
    start, count = run_of_xcd(x, nbig)
    if idx < count:
        return start + idx
    idx -= count
    start, count = run_of_xcd(x, nsmall)
    return nbig + start + idx if idx < count else -1


def queue_total(x, nbig, nsmall):
    return run_of_xcd(x, nbig)[1] + run_of_xcd(x, nsmall)[1]


def queue_first(block, nbig, nsmall):
    """workgroup `block`'s first tile, taken without an atomic: entry block / 8 of queue block % 8"""
    return queue_slot(block & 7, nbig, nsmall, block >> 3)


def head_preset(grid):
    """what conv0 writes into the 8 heads of a launch of `grid` workgroups: the entries the workgroups' first tiles have used"""
    return [(grid - x + 7) >> 3 for x in range(8)]


def nonempty_runs(nbig, nsmall):
    return sum(queue_total(x, nbig, nsmall) > 0 for x in range(8))


def drain(nbig, nsmall, grid, rng=None):
    """Every tile id a launch hands out, in one order of pulls and steals: the workgroups' first tiles, then, until every live workgroup
    has seen -1, a workgroup chosen by `rng` (None: round robin) pulls from its own queue or, that exhausted, tries the others from
    its neighbour on -- each try an atomic increment, successful or not, as in queue_publish.  -> the list of ids handed out."""
    heads = head_preset(grid)
    handed, live = [], []
    for b in range(grid):
        t = queue_first(b, nbig, nsmall)
        if t >= 0:  # (a workgroup whose first entry lies past its queue's end returns at once)
            handed.append(t)
            live.append(b)
    turn = 0
    while live:
        k = int(rng.integers(len(live))) if rng is not None else turn % len(live)
        turn += 1
        xcd = live[k] & 7
        t = queue_slot(xcd, nbig, nsmall, heads[xcd])
        heads[xcd] += 1
        if t < 0:
            snapshot = list(heads)
            for j in range(1, 8):
                x = (xcd + j) & 7
                if snapshot[x] >= queue_total(x, nbig, nsmall):
                    continue  # heads only grow: nothing there
                t = queue_slot(x, nbig, nsmall, heads[x])
                heads[x] += 1
                if t >= 0:
                    break
        if t < 0:
            live.pop(k)
        else:
            handed.append(t)
    return handed


def tile_coords(t, tiles_x, tiles_y, bw):
    """tile id within a class -> (image, tile column, tile row): column blocks of bw tile columns, each walked row by row
    (sr_kernels.h TileGrid, sr_kernels.hip tile_coords; bw <= 0 or >= tiles_x: plain row-major)"""
    tpi = tiles_x * tiles_y
    n, r = divmod(t, tpi)
    if bw <= 0 or bw >= tiles_x:
        ty, tx = divmod(r, tiles_x)
        return n, tx, ty
    nfull = tiles_x // bw
    b = min(r // (bw * tiles_y), nfull)
    rr = r - b * bw * tiles_y
    wide = bw if b < nfull else tiles_x - nfull * bw
    ty = rr // wide
    return n, b * bw + rr - ty * wide, ty


# ---- the table ----
def _case(cus, precision, h, w, reach, factor=3, io="f32", call="dev", n=1, halo=(0, 0), sets=None, ch=3, host=None):
    return {"cus": cus, "precision": precision, "h": h, "w": w, "reach": tuple(reach), "factor": factor, "io": io, "call": call, "n": n,
            "halo": list(halo), "set": dict(sets or {}), "ch": ch if io == "u8" else 3, "host": host,
            "pipeline": True, "profiling": False, "engines": 1, "oracle": h * w <= 61 * 97}


def _table():
    t = []
    both = ("f32", "u8")  # a device call's plan does not depend on its I/O kind: the rows of the issue in both
    Q, M, O, D, F, C0, CT = PROPERTIES
    # -- exact f32, factor 3: the production plans in miniature
    for io in both:
        t += [_case(1, "f32", 24, 33, [Q, M, O], io=io),                 # stages 1 and 3: 2 + 2 tile rows on 2 workgroups, queues 2-7 ownerless
              _case(1, "f32", 40, 70, [F, Q, M, O, C0], io=io),          # forks 18 / 22 by the rule
              _case(1, "f32", 61, 97, [F, Q, M, O, C0], io=io, ch=4),    # forks 30 / 31
              _case(3, "f32", 40, 70, [Q, O], io=io),                    # undivided, 15 tiles on 6 workgroups
              _case(5, "f32", 61, 97, [Q, M], io=io, ch=4),              # 6 + 4 tile rows x 4 columns on 10 workgroups: every XCD owned
              _case(2, "f32", 24, 33, [CT], io=io),                      # the controls: first form
              _case(5, "f32", 40, 70, [CT], io=io)]
    t += [_case(2, "f32", 100, 130, [F, Q, M, O, C0]),
          _case(3, "f32", 100, 130, [F, Q, M, O, C0], io="u8"),
          _case(3, "f32", 24, 33, [CT]),
          _case(5, "f32", 24, 33, [CT], io="u8", ch=4),
          _case(2, "f32", 40, 70, [F, Q, M, O])]
    # -- split-half, factor 3: 8-row tiles, up to 32 tiles through one workgroup
    for cus, io in zip((1, 2, 3, 5), ("f32", "u8", "f32", "u8")):
        t.append(_case(cus, "split_f16", 100, 130, [Q, C0] + ([O] if cus < 4 else []) + ([D] if cus < 3 else []), io=io, ch=4))
    for cus, (h, w) in itertools.product((1, 2, 3, 4, 5), ((24, 33), (40, 70), (61, 97))):
        io = both[(cus + h) % 2]
        single = 2 * cus >= ((h + 7) // 8) * ((w + 31) // 32)
        t.append(_case(cus, "split_f16", h, w, [CT] if single else [Q] + ([O] if cus < 4 else []), io=io))
    t += [_case(1, "split_f16", 61, 97, [Q, O, D, C0], io="u8", ch=4)]    # 32 tiles on 2 workgroups, on an image the oracle takes
    # -- factors 2 and 4: the final stage's other forms (the split-half mode's factor 4 has 4-row tiles only in its last stage)
    for factor, prec in itertools.product((2, 4), PRECISIONS):
        t += [_case(1, prec, 40, 70, ([F, M] if prec == "f32" else []) + [Q, O, C0], factor=factor),
              _case(5, prec, 61, 97, [Q] + ([M] if prec == "f32" else []), factor=factor, io="u8", ch=4),
              _case(5, prec, 24, 33, [Q] if (prec, factor) == ("split_f16", 4) else [CT], factor=factor, io="u8")]  # (its 12 4-row tiles on 10 workgroups)
    # -- batches: tile ids run across images
    for prec in PRECISIONS:
        t += [_case(1, prec, 24, 33, [Q, O] + ([M] if prec == "f32" else []), n=2),
              _case(2, prec, 24, 33, [Q, O], n=3, io="u8", ch=4),
              _case(2, prec, 40, 70, [Q, O, C0] + ([M] if prec == "f32" else []), n=2, factor=4),
              _case(1, prec, 13, 40, [Q, O], n=3, factor=2, io="u8")]
    # -- bands with halos
    for prec, halo in itertools.product(PRECISIONS, ((7, 7), (7, 0), (0, 7))):
        t.append(_case(1 if halo != (7, 0) else 2, prec, 54 if halo == (7, 7) else 47, 70, [Q, O] + ([C0] if halo != (7, 0) else []) + ([F, M] if prec == "f32" else []),
                       call="band", halo=halo, io="u8" if halo == (0, 7) else "f32"))
    # -- the switch matrix
    for prec in PRECISIONS:
        f32 = prec == "f32"
        for th in ("8", "4", FIVE):
            t.append(_case(1, prec, 40, 70, [Q, O, C0], sets={"th": th, "pipe": "all", "fork": "0"}))
        t.append(_case(5, prec, 24, 33, [Q], sets={"th": FIVE, "pipe": "all"}, io="u8"))
        for tail in ("0", "1", "2"):
            t.append(_case(2, prec, 61, 97, [Q, O, C0] + ([M] if tail != "0" else []), sets={"tail": tail, "fork": "0"}))
        t.append(_case(5, prec, 100, 130, [Q, M, C0], sets={"tail": "1", "fork": "0"}, io="u8"))
        for bw in ("0", "1", "2"):
            t += [_case(2, prec, 40, 130, [Q, O, C0] + ([M] if f32 else []), sets={"bw": bw, "fork": "0"}),          # 5 tile columns
                  _case(1, prec, 29, 70, [Q, O, C0] + ([M] if f32 else []), sets={"bw": bw}, n=2, io="u8", ch=4)]    # 3 tile columns, two images
        for fork in ("0", "1", "14"):
            t.append(_case(1, prec, 61, 97, [Q, O, C0] + ([F] if fork != "0" else [D]) + ([M] if f32 and fork != "14" else []), sets={"fork": fork}))
    for wino in ("0", "2"):  # ("": every other f32 case)
        t += [_case(1, "f32", 40, 70, [F, Q, M, O, C0], sets={"wino": wino}),
              _case(5, "f32", 61, 97, [Q, M], sets={"wino": wino}, io="u8")]
    # -- host-pointer calls: bands of a tiny image, in order on one stream and on alternating ones
    for prec in PRECISIONS:
        t += [_case(1, prec, 40, 70, [Q, O], call="host", sets={"rows": "20,20"}, host="inorder"),
              _case(2, prec, 61, 97, [Q, O] + ([M] if prec == "f32" else []), call="host", sets={"rows": "=20,21,20"}, host="alternating", io="u8", ch=4),
              _case(1, prec, 24, 33, [Q, O], call="host", n=3, io="u8")]
    for k, c in enumerate(t):
        c["id"] = k
        c["name"] = (f"{k:03d}-cus{c['cus']}-{c['precision']}-f{c['factor']}-{c['call']}-{c['io']}{c['ch'] if c['io'] == 'u8' else ''}-"
                     f"{c['n']}x{c['h']}x{c['w']}" + ("-halo%d.%d" % tuple(c["halo"]) if any(c["halo"]) else "") +
                     "".join(f"-{key}={v}" for key, v in c["set"].items()))
    return t


TABLE = _table()


def by_cus(cases=None):
    out = {}
    for c in TABLE if cases is None else cases:
        out.setdefault(c["cus"], []).append(c)
    return out


def planner_view(case):
    """the case as plan_cases.check_line takes it: without the switches no planner reads ("bw" orders the tile ids inside the kernel)"""
    return {**case, "set": {k: v for k, v in case["set"].items() if k != "bw"}}


def plan_table(exe, cases=None):
    """{case id: the HIP-free planner's lines of the case's one context}, each case planned for its own compute units"""
    import plan_cases
    out = {}
    for cus, group in sorted(by_cus(cases).items()):
        status, err, planned = plan_cases.run_plan_check(exe, [planner_view(c) for c in group], cus)
        assert status == 0, err
        for c in group:
            assert len(planned[c["id"]]) == 1, c["name"]
            out[c["id"]] = planned[c["id"]][0]
    return out


# ---- what the planner's lines say a case reaches ----
def launches_of(ctx_lines):
    """plan_check's lines of one context -> [(st, form, ty8, ty4, grid, y0, y1)] in issue order"""
    out, rows = [], None
    for l in ctx_lines:
        w = l.split()
        if l.startswith("# rows"):
            rows = (int(w[2]), int(w[3]))
        elif w[0] == "launch":
            out.append((int(w[1]), w[2], int(w[3]), int(w[4]), int(w[5]), *rows))
    return out


def _images(case, ctx_lines):
    """images of the k-th launch's pass: a host call's batch chunks differ (five launches a pass), everything else runs the call's n"""
    for l in ctx_lines:
        if l.startswith("host batch"):
            sizes = [int(v) for v in l.split()[2].split(",")]
            return lambda k: sizes[k // 5]
    return lambda k: case["n"]


def queue_launches(case, ctx_lines):
    """(nbig, nsmall, grid) of every pipe launch of the case that asks the queue (fewer workgroups than tiles)"""
    tx = (case["w"] + 31) // 32
    n_of = _images(case, ctx_lines)
    out = []
    for k, (st, form, ty8, ty4, grid, y0, y1) in enumerate(launches_of(ctx_lines)):
        if st > 0 and form == "pipe" and grid < n_of(k) * tx * (ty8 + ty4):
            out.append((n_of(k) * tx * ty8, n_of(k) * tx * ty4, grid))
    return out


def reached(case, ctx_lines):
    """-> the set of PROPERTIES the planner's lines of the case show"""
    tx = (case["w"] + 31) // 32
    n_of = _images(case, ctx_lines)
    launches = launches_of(ctx_lines)
    assert launches and len(launches) % 5 == 0, ctx_lines
    got = set()
    if any(st == 0 and n_of(k) * tx * (ty8 + ty4) > 8 * case["cus"] for k, (st, _, ty8, ty4, *_) in enumerate(launches)):
        got.add("conv0-rounds")
    asking = queue_launches(case, ctx_lines)
    for nbig, nsmall, grid in asking:
        got.add("queue")
        if nbig and nsmall:
            got.add("mixed")
        if grid < 8 and nonempty_runs(nbig, nsmall) > grid:
            got.add("ownerless")
        if nbig + nsmall >= 16 * grid:
            got.add("deep")
    if any(l.startswith("fork 1") for l in ctx_lines):
        got.add("fork")
    if not asking:
        got.add("control")
    return got
