"""What the host decides about a GAN step (csrc/ndp_capi.inc: the network tables g_mlp / d_mlp, step_plan, build_jobs,
fill_reduce), before anything runs on a GPU: a wrong chunk count, grid, offset or job field is a launch that reads or writes
out of bounds or sums the wrong slabs, not a failing result.  tests/host_drivers/step_plan.inc reports, per query, the
plan, the parameter layouts and packed-copy offsets, the 12 workspace offsets, the workspaces' tensors, every field of every
WgradJob of both networks (pointers named by the tensor they lie in) and the regions of both reduces.

tests/golden/step_launch_plan.json holds the same reports as the host code gave them before the plan was one struct and
the job builder one function: layouts, workspace sizes and offsets, job tables, chunk and slab counts and reduce regions
from the functions that computed them then; the grids, the phase kernels' template choice, the heavy / light mark -> count
of launch_wgrad and every loss_count transcribed from the expressions that stood beside the launches.  TABLE restates the
thresholds a third time, by hand, for the shapes of the GPU gradient suite.

Host arithmetic only; the program is host_driver's, an ordinary child process under AddressSanitizer and UBSan."""
import json
import os
import struct

import numpy as np
import pytest

import host_driver
from test_gpu_step_gradients import SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
PLAN = ("m mpad rpad d_rows g_heavy g_light g_wide g_slabs d_heavy d_light d_wide d_slabs seg_per_tile seg_entries ndiv_fused "
        "ndiv_threads ndiv_blocks d_front_grid a_ring a_nr phase_b_grid b_ring b_pre b_nr wgrad_d_grid wgrad_d_wide wgrad_g_grid "
        "wgrad_g_wide reduce_d_grid reduce_g_grid ndiv_grid pack_g_grid pack_d_grid loss_count_d loss_count_g loss_count_ndiv "
        "floats").split()
REGIONS = ("g.h1 g.h2 g.h3 g.h4 g.dy1 g.dy2 g.dy3 g.dy4 g.dy5 g.slabs d.xa d.h1 d.h2 d.h3 d.dy1 d.dy2 d.dy3 d.dl d.slabs d.lossp "
           "d_action nd_grad nd_part g_packed d_packed d_seg g_seg").split()
JOB = ("a_space a_off b_space b_off lda ldb a_cols b_cols b_rowmod b_rowdiv b_rowmax b_vec dst_off dst_ld bias_off kind rows seg "
       "seg_s seg_k seg_wrap nchunks").split()
WG_WIDE = 3
CODES, NOISE = 1, 2                                           # the driver's spaces beside the workspaces
WIDTHS = {"g": lambda nz: (256 + nz, 128, 64, 128, 256, 4), "d": lambda nz: (260, 64, 128, 256, 1)}
REPEAT = (64, 6, 2)                                           # the shape whose repeat D step the GPU suite runs


def step(batch, k, nz, first=1):
    return (0, 7 * batch, k, nz, first)


# (kind, flat or m, K, nz, first): the GPU suite's shapes, first and repeat D step; both sides of every threshold (row
# counts are multiples of 32 and phase grids even, so "257 workgroups" is 258); the module-level backward calls
QUERIES = [step(*s, first=f) for s in SHAPES for f in (1, 0)] + [
    (0, 32, 127, 2, 1), (0, 32, 128, 2, 1),                   # D rows 4,096 / 4,128 = 256 / 258 workgroups of k_phase_a
    (0, 64, 32, 2, 0), (0, 65, 32, 2, 0),                     # repeat D step: 4,096 / 4,160 rows
    (0, 128, 32, 2, 1), (0, 129, 32, 2, 1),                   # 256 / 258 workgroups of k_phase_b
    (0, 511, 32, 2, 1), (0, 512, 32, 2, 1),                   # G rows 16,352 / 16,384
    (0, 65, 250, 2, 1), (0, 64, 255, 2, 1),                   # D rows 16,352 / 16,384
    (0, 874, 32, 2, 1), (0, 875, 32, 2, 1),                   # G rows 27,968 / 28,000
    (0, 110, 253, 2, 1), (0, 111, 251, 2, 1),                 # D rows 27,968 / 28,000
    (0, 448, 6, 3, 1),                                        # nz 3 beside (64, 6, 2): NDiv leaves the D launch
    (0, 1000, 5, 2, 1), (0, 1000, 6, 2, 1), (0, 1000, 16, 2, 1),   # K 5 / 6 / 16 on the small rings: NR 0 / 4 / 1
    (1, 1, 1, 2, 0), (1, 33, 1, 2, 0), (1, 245, 1, 2, 0), (1, 245, 7, 5, 0),
]

# The thresholds restated by hand for SHAPES: M, pad M, D rows, G heavy/light, D heavy/light, wide chunks G/D, k_phase_a
# (workgroups, ring, NR), k_phase_b (workgroups, ring, NR), seg_per_tile, NDiv fused
TABLE = {
    (5, 7, 2): (245, 256, 320, 4, 4, 5, 5, 0, 0, 20, 96, 0, 16, 96, 0, 4, 1),
    (25, 6, 2): (1050, 1056, 1248, 16, 16, 8, 8, 0, 0, 78, 96, 0, 66, 96, 0, 4, 1),
    (64, 6, 2): (2688, 2688, 3136, 24, 12, 8, 8, 0, 0, 196, 96, 0, 168, 96, 0, 4, 1),
    (52, 6, 2): (2184, 2208, 2592, 24, 12, 8, 8, 0, 0, 162, 96, 0, 138, 96, 0, 4, 1),
    (72, 6, 2): (3024, 3040, 3552, 24, 12, 8, 8, 0, 0, 222, 96, 0, 190, 96, 0, 4, 1),
    (98, 6, 2): (4116, 4128, 4832, 24, 12, 32, 8, 0, 0, 302, 24, 4, 258, 32, 4, 4, 1),
    (200, 3, 2): (4200, 4224, 5632, 24, 12, 32, 8, 0, 0, 352, 24, 0, 264, 32, 0, 7, 1),
    (24, 32, 2): (5376, 5376, 5568, 24, 12, 32, 8, 0, 0, 348, 24, 1, 336, 32, 1, 2, 1),
    (392, 6, 2): (16464, 16480, 19232, 32, 32, 32, 32, 0, 0, 1202, 24, 4, 1030, 32, 4, 4, 1),
    (128, 32, 2): (28672, 28672, 29568, 32, 32, 32, 32, 64, 64, 1848, 24, 1, 1792, 32, 1, 2, 1),
    (672, 6, 2): (28224, 28224, 32928, 32, 32, 32, 32, 64, 64, 2058, 24, 4, 1764, 32, 4, 4, 1),
    (40, 5, 5): (1400, 1408, 1696, 16, 16, 8, 8, 0, 0, 106, 96, 0, 88, 96, 0, 5, 0),
    (40, 6, 1): (1680, 1696, 1984, 24, 12, 8, 8, 0, 0, 124, 96, 0, 106, 96, 0, 4, 1),
}
TABLE_FIELDS = ("m mpad d_rows g_heavy g_light d_heavy d_light g_wide d_wide d_front_grid a_ring a_nr phase_b_grid b_ring b_nr "
                "seg_per_tile ndiv_fused").split()


def decode(v):
    """One report of the driver (kind 0 or 1) as a dict; returns it and the number of values read."""
    at = [0]

    def take(n):
        at[0] += n
        return [int(x) for x in v[at[0] - n:at[0]]]
    r = {"plan": dict(zip(PLAN, take(len(PLAN))))}
    for net in "gd":
        o = take(20)
        r[net] = {"w": o[0:5], "b": o[5:10], "total": o[10], "pack_fwd": o[11:15], "pack_dg": o[15:19], "pack_total": o[19]}
    r["offsets"] = take(12)
    r["regions"] = {name: tuple(take(3)) for name in REGIONS}
    for net in "gd":
        njobs, nwide, wide_chunks, nchunks = take(4)
        r[net].update(njobs=njobs, nwide=nwide, wide_chunks=wide_chunks, nchunks=nchunks,
                      jobs=[dict(zip(JOB, take(len(JOB)))) for _ in range(njobs + nwide)])
    for net in "gd":
        slabs, n, nreg = take(3)
        r[net]["reduce"] = {"slabs": slabs, "n": n, "regions": [tuple(take(3)) for _ in range(4)][:nreg]}
    return r, at[0]


def ask(queries, work_dir):
    payload = struct.pack("<i", len(queries)) + b"".join(struct.pack("<5i", *q) for q in queries)
    raw = host_driver.run("step_plan", payload, work_dir, exe=host_driver.build())
    return np.frombuffer(raw, dtype="<i8")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "step_launch_plan.json")) as f:
        doc = json.load(f)
    assert doc["plan"] == list(PLAN) and doc["regions"] == list(REGIONS) and doc["job"] == list(JOB)
    return {tuple(q): r for q, r in zip(doc["queries"], doc["reports"])}


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    v = ask(QUERIES, tmp_path_factory.mktemp("step_plan"))
    out, at = {}, 0
    for q in QUERIES:
        r, n = decode(v[at:])
        out[q] = (r, [int(x) for x in v[at:at + n]])
        at += n
    assert at == len(v)
    return out


def test_every_report_equals_the_recorded_one(golden, reports):
    assert set(golden) == set(QUERIES)
    for q in QUERIES:
        got, raw = reports[q]
        if raw != golden[q]:                                   # name the first field that differs
            want, _ = decode(golden[q])
            for part in ("plan", "offsets", "regions"):
                assert got[part] == want[part], (q, part)
            for net in "gd":
                for key in want[net]:
                    if key != "jobs":
                        assert got[net][key] == want[net][key], (q, net, key)
                for i, (a, b) in enumerate(zip(got[net]["jobs"], want[net]["jobs"])):
                    assert a == b, (q, net, "job", i)
        assert raw == golden[q], q


def test_the_hand_written_table_agrees(reports):
    assert set(TABLE) == set(SHAPES)
    for s in SHAPES:
        plan = reports[step(*s)][0]["plan"]
        assert tuple(plan[k] for k in TABLE_FIELDS) == TABLE[s], s
        assert (plan["b_pre"] == 1) == (plan["b_ring"] == 96), s
    plan = reports[step(*REPEAT, first=0)][0]["plan"]          # the repeat D step: two full passes
    assert (plan["d_rows"], plan["d_heavy"], plan["d_light"], plan["d_wide"], plan["a_ring"]) == (5376, 32, 8, 0, -1)
    assert plan["d_front_grid"] == plan["loss_count_d"] == 2688 // 16


def branch(rows, heavy, light):
    return "uniform from 16,384 rows" if rows >= 16384 else ("uniform small" if heavy == light else "heavy / light")


def test_the_gpu_suites_shapes_reach_every_variant_and_branch(reports, tmp_path):
    v = [int(x) for x in ask([(3, 0, 0, 0, 0)], tmp_path)]
    list_a = {tuple(v[1 + 2 * i:3 + 2 * i]) for i in range(v[0])}
    at = 1 + 2 * v[0]
    list_b = {tuple(v[at + 1 + 3 * i:at + 4 + 3 * i]) for i in range(v[at])}
    assert len(list_a) == v[0] == 4 and len(list_b) == v[at] == 4 and at + 1 + 3 * v[at] == len(v)
    plans = [reports[step(*s)][0]["plan"] for s in SHAPES] + [reports[step(*REPEAT, first=0)][0]["plan"]]
    first = plans[:-1]
    assert {(p["a_ring"], p["a_nr"]) for p in first} == list_a
    assert {(p["b_ring"], p["b_pre"], p["b_nr"]) for p in first} == list_b
    for net in "gd":
        assert {p["wgrad_%s_wide" % net] for p in plans} == {0, 1}, net    # k_wgrad and k_wgrad_wide
    assert {p["ndiv_fused"] for p in plans} == {0, 1}
    assert {p["ndiv_grid"] > 0 for p in plans} == {False, True}
    want = {"uniform small", "heavy / light", "uniform from 16,384 rows"}
    assert {branch(p["mpad"], p["g_heavy"], p["g_light"]) for p in plans} == want
    assert {branch(p["d_rows"], p["d_heavy"], p["d_light"]) for p in plans} == want


def contains(region, space, begin, end):
    return region[0] == space and region[1] <= begin and end <= region[2]


def test_each_report_is_consistent_in_itself(reports):
    for q in QUERIES:
        r, _ = reports[q]
        kind, flat, k, nz, _ = q
        plan, regions = r["plan"], dict(r["regions"])
        m = plan["m"]
        regions["codes"] = (CODES, 0, (flat if kind == 0 else m) * 256)
        regions["noise"] = (NOISE, 0, m * nz)
        # the workspace: its tensors in order, none overlapping, the last one ending where the workspace ends
        if kind == 0:
            spans = sorted(v[1:] for v in r["regions"].values())
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), q
            assert spans[0][0] == 0 and spans[-1][1] == plan["floats"], q
            assert r["offsets"][:4] == [r["regions"]["g.h%d" % i][1] for i in range(1, 5)], q
            assert r["offsets"][4:6] == [r["regions"]["nd_grad"][1], r["regions"]["g.dy5"][1]], q
            at = 6 if q[4] else 9                              # D's h1..h3 in this D step's layout of its scratch
            assert r["offsets"][at:at + 3] == [r["regions"]["d.h%d" % i][1] for i in range(1, 4)], q
            assert plan["loss_count_d"] == plan["d_front_grid"] and plan["loss_count_g"] == plan["phase_b_grid"], q
            assert r["regions"]["d.lossp"][2] - r["regions"]["d.lossp"][1] >= plan["loss_count_d"], q
            assert r["regions"]["nd_part"][2] - r["regions"]["nd_part"][1] >= plan["loss_count_ndiv"], q
        for net in "gd":
            n = r[net]
            widths = WIDTHS[net](nz)
            layers = len(widths) - 1
            rows = plan["mpad"] if net == "g" or kind == 1 else plan["d_rows"]
            heavy, light, wide, slabs = (plan["%s_%s" % (net, x)] for x in ("heavy", "light", "wide", "slabs"))
            # slab area = slab count x padded parameter count; the reduce sums what the jobs wrote
            area = r["regions"][net + ".slabs"]
            assert area[2] - area[1] == slabs * ((n["total"] + 3) // 4 * 4), (q, net)
            assert slabs == max(heavy, wide) and n["nchunks"] == n["reduce"]["slabs"] == heavy >= light, (q, net)
            assert n["reduce"]["n"] == n["total"] == n["b"][layers - 1] + widths[-1], (q, net)
            assert (n["nwide"], n["wide_chunks"]) == ((2, wide) if wide else (0, 0)), (q, net)
            grid = plan["wgrad_%s_grid" % net] - (plan["ndiv_blocks"] if net == "d" and kind == 0 and plan["ndiv_fused"] else 0)
            assert grid == n["nwide"] * n["wide_chunks"] + 8 * ((heavy + 7) // 8) * n["njobs"], (q, net)
            assert plan["reduce_%s_grid" % net] == (n["total"] + 255) // 256 + 1, (q, net)
            weights, biases = np.zeros(n["total"], dtype=np.int32), np.zeros(n["total"], dtype=np.int32)
            chunks_of = {}
            for i, j in enumerate(n["jobs"]):
                where = (q, net, i)
                # the destination block inside its layer's parameters
                layer = max(l for l in range(layers) if n["w"][l] <= j["dst_off"])
                out, inp = widths[layer + 1], widths[layer]
                assert j["dst_ld"] == inp and j["lda"] == out, where
                row0, col0 = divmod(j["dst_off"] - n["w"][layer], inp)
                assert row0 + j["a_cols"] <= out and col0 + j["b_cols"] <= inp, where
                block = n["w"][layer] + (row0 + np.arange(j["a_cols"]))[:, None] * inp + col0 + np.arange(j["b_cols"])[None, :]
                weights[block.ravel()] += 1
                if j["bias_off"] >= 0:
                    assert j["bias_off"] == n["b"][layer] + row0, where
                    biases[j["bias_off"]:j["bias_off"] + j["a_cols"]] += 1
                assert (j["kind"] == WG_WIDE) == (i >= n["njobs"]), where
                assert j["nchunks"] in (heavy, light, wide) and 1 <= j["nchunks"] <= slabs, where
                chunks_of.setdefault(layer, set()).add(j["nchunks"])
                # the operands inside the tensors they are named after, for the rows the job runs over
                jrows = j["rows"] or rows
                a_end = j["a_off"] + (jrows - 1) * j["lda"] + j["a_cols"]
                a_name = ("d_seg" if net == "d" else "g_seg") if j["seg"] else "%s.dy%d" % (net, layer + 1)
                if a_name == "d.dy4":
                    a_name = "d.dl"
                assert contains(regions[a_name], j["a_space"], j["a_off"], a_end), where + (a_name,)
                if j["seg"]:
                    assert j["seg_s"] == plan["seg_per_tile"] and j["seg_k"] == k, where
                    assert jrows == plan["seg_entries"] + (plan["rpad"] if net == "d" else 0), where
                    assert j["seg_wrap"] == (plan["seg_entries"] if net == "d" else 0), where
                last = min((min(jrows, j["b_rowmod"]) - 1) // j["b_rowdiv"], j["b_rowmax"])
                if j["seg"]:
                    last = j["b_rowmax"]
                b_end = j["b_off"] + last * j["ldb"] + j["b_cols"]
                if layer > 0:
                    b_name = "%s.h%d" % (net, layer)
                elif j["b_cols"] == 64:
                    b_name = "codes"
                else:
                    b_name = "noise" if net == "g" else "d.xa"
                assert contains(regions[b_name], j["b_space"], j["b_off"], b_end), where + (b_name,)
                assert j["b_vec"] == (j["ldb"] % 4 == 0 and j["b_off"] % 4 == 0), where
            # every parameter written exactly once: weights and biases counted separately
            is_bias = np.zeros(n["total"], dtype=bool)
            for l in range(layers):
                is_bias[n["b"][l]:n["b"][l] + widths[l + 1]] = True
            assert (weights[~is_bias] == 1).all() and (weights[is_bias] == 0).all(), (q, net)
            assert (biases[is_bias] == 1).all() and (biases[~is_bias] == 0).all(), (q, net)
            assert n["njobs"] + (8 if wide else 0) == {"g": 26, "d": 19}[net], (q, net)
            # one chunk count per layer, and the reduce's regions say which layers have fewer slabs than `heavy`
            want = []
            for l in sorted(chunks_of):
                assert len(chunks_of[l]) == 1, (q, net, l)
                (c,) = chunks_of[l]
                if c != heavy:
                    want.append((n["w"][l], n["b"][l] + widths[l + 1], c))
            assert sorted(n["reduce"]["regions"]) == sorted(want), (q, net)


REFUSED = [(2, 0, 0, 0, -1), (2, 448, 0, 2, 0), (2, 448, 257, 2, 0), (2, 448, 6, 0, 0), (2, 448, 6, 17, 0), (2, 0, 6, 2, 0),
           (2, 1 << 20, 256, 2, 0)]                            # null; num_sample 0, 257; noise_dim 0, 17; flat 0; flat x K = 2^28


@pytest.mark.parametrize("query", REFUSED)
def test_every_step_entry_point_refuses_a_bad_configuration(query, tmp_path):
    floats, offset, d_grads, g_grads, pack, adam = (int(x) for x in ask([query], tmp_path))
    assert (floats, offset) == (0, -1)
    assert d_grads == g_grads == pack == adam == 1             # NDP_E_ARG

