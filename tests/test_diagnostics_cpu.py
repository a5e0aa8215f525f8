"""Calibration and 2-D mode statistics without a device: the pure-numpy states of cgs_amd.metrics against goldens recorded from the
reference's calibration_diagnostic / calibration_bins / metrics_distance / freq_category (tests/golden/make_calibration_golden.py), the
state algebra, the C ABI surface of csrc/diagnostics.hip, the two row formatters and the all-reduce of states over gloo."""
import os
import re
import socket

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["cgs_calibration_ws_bytes", "cgs_calibration_accumulate", "cgs_mode_stats_ws_bytes", "cgs_mode_stats_accumulate"]


@pytest.fixture(scope="module")
def cal():
    return np.load(os.path.join(GOLDEN, "calibration_golden.npz"))


@pytest.fixture(scope="module")
def modes():
    return np.load(os.path.join(GOLDEN, "mode_golden.npz"))


def _whole(g, case):
    from cgs_amd.metrics import calibration_merge, calibration_state_of
    return calibration_merge(calibration_state_of(g[f"{case}_fake"], 0), calibration_state_of(g[f"{case}_real"], 1))


# ---------------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("case", ["c1", "c2", "c3"])
def test_states_reproduce_the_reference_diagnostics_and_bins(cal, case):
    from cgs_amd.metrics import calibration_diagnostics
    d = calibration_diagnostics(_whole(cal, case))
    for got, want in ((d["accuracy"], cal[f"{case}_prob_true"]), (d["confidence"], cal[f"{case}_prob_pred"]), (d["weights"], cal[f"{case}_weights"])):
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
    got = np.array([d["z_dawid"], d["brier"], d["ece"], d["mce"]])
    assert np.abs(got - cal[f"{case}_diag"]).max() <= 1e-9, (got, cal[f"{case}_diag"])
    real = cal[f"{case}_real"].astype(np.float64)
    assert d["real_max"] == real.max() and abs(d["real_mean"] - real.mean()) <= 1e-15


def test_edge_neighbours_fall_into_the_slots_of_np_digitize_in_double(cal):
    from cgs_amd.metrics import calibration_edges, calibration_state_of
    edges = calibration_edges(20)
    assert np.array_equal(edges, cal["edges"])
    for label, key in ((0, "c2_fake"), (1, "c2_real")):
        p = cal[key]
        st = calibration_state_of(p, label)
        want = np.bincount(np.digitize(p.astype(np.float64), edges) - 1, minlength=21)
        assert np.array_equal(st["count"], want) and st["under"] == 0 and st["n"] == p.size
    # the trap the double comparison avoids: fp32(0.05) lies above the edge 0.0500000005, the double 0.05 below it
    assert calibration_state_of(np.float32(0.05), 0)["count"][1] == 1
    assert np.digitize(np.float32(0.05), edges.astype(np.float32)) - 1 == 1 and np.digitize(0.05, edges) - 1 == 0


# ---------------------------------------------------------------------------------------------------------------- calibration algebra
def _same_state(a, b, tol=0.0):
    assert set(a) == set(b)
    for k in a:
        if k in ("sum_p", "sum_y", "sum_ymp", "sum_var", "sum_sq", "label_sum"):
            assert np.abs(np.asarray(a[k]) - np.asarray(b[k])).max() <= tol * max(1.0, np.abs(np.asarray(b[k])).max()), k
        else:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("cuts", [(0, 1, 2500), (0, 700, 1000, 1900, 2500), (0, 2500, 2500)])
def test_merge_of_any_split_equals_the_whole(cal, cuts):
    from cgs_amd.metrics import calibration_merge, calibration_state_of
    p = np.concatenate([cal["c1_fake"], cal["c1_real"]])
    y = np.concatenate([np.zeros(1000, int), np.ones(1500, int)])
    whole = _whole(cal, "c1")
    st = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        for label in (0, 1):
            part = calibration_state_of(p[a:b][y[a:b] == label], label)
            st = part if st is None else calibration_merge(st, part)
    _same_state(st, whole, tol=1e-13)
    with pytest.raises(ValueError):
        calibration_merge(whole, calibration_state_of(p, 0, n_bins=10))


def test_scores_below_the_first_edge_are_counted_and_refused_nan_and_large_land_in_the_last_slot():
    from cgs_amd.metrics import calibration_diagnostics, calibration_state_of
    st = calibration_state_of(np.array([0.25, np.nan, 1.5, 0.75], dtype=np.float32), 1)
    assert st["count"][20] == 2 and st["count"].sum() == st["n"] == 4 and st["under"] == 0
    assert st["label_max"][1] == 1.5                                  # a NaN never wins the maximum
    st = calibration_state_of(np.array([0.25, -0.25, -1e-30], dtype=np.float32), 0)
    assert st["under"] == 2 and st["n"] == 1 and st["sum_p"].sum() == 0.25
    with pytest.raises(ValueError):
        calibration_diagnostics(st)
    for bad in (dict(label=2), dict(label=0, n_bins=0), dict(label=0, n_bins=65)):
        with pytest.raises(ValueError):
            calibration_state_of(np.zeros(3, np.float32), **bad)


def test_flat_device_layout_round_trips(cal):
    from cgs_amd.metrics import _cal_flat, _cal_unflat
    st = _whole(cal, "c2")
    h = _cal_flat(st)
    assert h.shape == (3 * 21 + 11,) and h[3 * 21] == st["n"] and h[3 * 21 + 5 + 3] == 1503 and h[-1] == st["label_max"][1]
    _same_state(_cal_unflat(h, 20), st)


# ---------------------------------------------------------------------------------------------------------------- modes
@pytest.mark.parametrize("tag", ["g25", "imb8"])
def test_mode_states_equal_the_whole_array_functions_and_the_reference(modes, tag):
    from cgs_amd import metrics as M
    c, thres, real, model = modes[f"{tag}_centeroids"], float(modes[f"{tag}_thres"][0]), modes[f"{tag}_real"], modes[f"{tag}_model"]
    sr, sm = M.mode_state_of(real, c, thres), M.mode_state_of(model, c, thres)
    # a three-way split merges to the same counts
    parts = M.mode_merge(M.mode_merge(M.mode_state_of(model[:1], c, thres), M.mode_state_of(model[1:600], c, thres)), M.mode_state_of(model[600:], c, thres))
    assert np.array_equal(parts["counts"], sm["counts"]) and (parts["n"], parts["good"]) == (sm["n"], sm["good"])
    assert abs(parts["sum_min"] - sm["sum_min"]) <= 1e-12 * sm["sum_min"]
    got = M.mode_metrics(sm, sr)
    md, good = M.metrics_distance(model, c, thres)
    want = dict(mean_dist=md, good=good, kl=M.metrics_diversity(real, model, c, thres), js=M.metrics_distribution(real, model, c, thres))
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, k
    assert good * sm["n"] == sm["good"]
    hits = M._mode_distances(model, c) < thres
    assert np.array_equal(sm["counts"], hits.sum(axis=0))
    ref = np.concatenate([modes[f"{tag}_ref_model_dist"], modes[f"{tag}_ref_kl_js"]])
    assert np.abs(np.array([got["mean_dist"], got["good"], got["kl"], got["js"]]) - ref).max() <= 1e-12
    fv, fa = M._freqs_from_counts(sm["counts"], sm["n"])
    assert np.abs(fv - modes[f"{tag}_ref_model_freqs_valid"]).max() <= 1e-15 and np.abs(fa - modes[f"{tag}_ref_model_freqs_all"]).max() <= 1e-15


@pytest.mark.parametrize("tag", ["g25", "imb8"])
def test_existing_mode_metrics_keep_their_bits_after_the_helper_refactor(modes, tag):
    """``proj_*`` are what these functions returned on the commit before their count-to-frequency tail became shared helpers."""
    from cgs_amd import metrics as M
    c, thres, real, model = modes[f"{tag}_centeroids"], float(modes[f"{tag}_thres"][0]), modes[f"{tag}_real"], modes[f"{tag}_model"]
    for pool, x in (("real", real), ("model", model)):
        assert np.array_equal(np.array(M.metrics_distance(x, c, thres)), modes[f"{tag}_proj_{pool}_dist"])
        fv, fa = M.freq_category(x, c, thres)
        assert np.array_equal(fv, modes[f"{tag}_proj_{pool}_freqs_valid"]) and np.array_equal(fa, modes[f"{tag}_proj_{pool}_freqs_all"])
    got = np.array([M.metrics_diversity(real, model, c, thres), M.metrics_distribution(real, model, c, thres)])
    assert np.array_equal(got, modes[f"{tag}_proj_kl_js"])
    empty = M.freq_category(model + 1000.0, c, thres)                 # no hit at all: the uniform fallback
    assert np.array_equal(empty[0], np.ones(len(c)) / len(c)) and empty[1][-1] == 1.0


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_bindings_and_library_agree_on_the_new_entry_points():
    import ctypes
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    l = lib.load()
    for name in NEW:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        nargs = len(decl.group(1).split(","))
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    assert lib.SIGNATURES["cgs_calibration_ws_bytes"] == lib.SIGNATURES["cgs_mode_stats_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 2)
    assert lib.SIGNATURES["cgs_mode_stats_accumulate"][1][4] is ctypes.c_double
    assert l.cgs_version() >= 111
    assert "diagnostics.hip" in open(os.path.join(ROOT, "collaborative-gan-sampling_amd", "csrc", "Makefile")).read()
    assert lib.built_from() == lib.source_hash()                      # cgs_source_sha covers the new file


def plan(n):
    """csrc/diagnostics.hip, diag_plan restated: 512 elements per one-wave block, at most 1024 blocks, chunks of whole 64-lane rows."""
    blocks = min(-(-n // 512), 1024)
    chunk = -(-(-(-n // blocks)) // 64) * 64
    return chunk, -(-n // chunk)


@pytest.mark.parametrize("n,blocks", [(1, 1), (64, 1), (512, 1), (513, 2), (4099, 9), (70001, 137), (1 << 20, 1024), (1000000, 977)])
def test_workspace_queries_follow_the_restated_plan_and_bad_arguments_launch_nothing(n, blocks):
    from cgs_amd import lib
    l = lib.load()
    chunk, nb = plan(n)
    assert nb == blocks and chunk % 64 == 0 and (nb - 1) * chunk < n <= nb * chunk
    assert int(l.cgs_calibration_ws_bytes(n, 20)) == nb * (3 * 21 + 11) * 8
    assert int(l.cgs_mode_stats_ws_bytes(n, 25)) == nb * 28 * 8
    for bins in (0, 65):
        assert int(l.cgs_calibration_ws_bytes(n, bins)) == 0
        assert l.cgs_calibration_accumulate(None, n, 0, None, bins, None, None, 0, None) == lib.EINVAL     # null pointers: the check comes first
    for k in (0, 65):
        assert int(l.cgs_mode_stats_ws_bytes(n, k)) == 0
        assert l.cgs_mode_stats_accumulate(None, n, None, k, 1.0, None, None, 0, None) == lib.EINVAL
    assert l.cgs_calibration_accumulate(None, n, 2, None, 20, None, None, 0, None) == lib.EINVAL
    assert l.cgs_calibration_accumulate(None, -1, 0, None, 20, None, None, 0, None) == lib.EINVAL
    assert l.cgs_calibration_accumulate(None, n, 0, None, 20, None, None, 0, None) == lib.EINVAL            # n scores of a null p
    assert l.cgs_calibration_accumulate(None, 0, 1, None, 20, None, None, 0, None) == lib.OK                # no score: a no-op
    assert l.cgs_mode_stats_accumulate(None, 0, None, 8, 1.0, None, None, 0, None) == lib.OK


# ---------------------------------------------------------------------------------------------------------------- rows
def test_formatters_reproduce_the_recorded_rows_byte_for_byte(cal):
    from cgs_amd.evaluate import row_nsgan, row_synthetic
    a = cal["row_synthetic_args"]
    quality = dict(mean_dist=a[2], good=a[3], kl=a[4], js=a[5])
    diag = dict(z_dawid=a[7], brier=a[8], ece=a[9], mce=a[10])
    assert row_synthetic(int(a[0]), int(a[1]), quality, a[6], diag).encode() == cal["row_synthetic"].tobytes()
    b = cal["row_nsgan_args"]
    diag = dict(z_dawid=b[5], brier=b[6], ece=b[7], mce=b[8])
    assert row_nsgan(int(b[0]), int(b[1]), b[2], b[3], b[4], diag).encode() == cal["row_nsgan"].tobytes()
    assert cal["row_nsgan"].tobytes().endswith(b"\r\n") and cal["row_synthetic"].tobytes().count(b"    ") == 10


# ---------------------------------------------------------------------------------------------------------------- ranks
def test_all_reduce_without_a_process_group_is_the_identity(cal, modes):
    from cgs_amd.metrics import all_reduce_calibration, all_reduce_modes, mode_state_of
    st = _whole(cal, "c3")
    assert all_reduce_calibration(st) is st
    ms = mode_state_of(modes["g25_model"], modes["g25_centeroids"], 0.2)
    assert all_reduce_modes(ms) is ms


def _rank_inputs(rank):
    g, m = np.load(os.path.join(GOLDEN, "calibration_golden.npz")), np.load(os.path.join(GOLDEN, "mode_golden.npz"))
    fake, real = g["c1_fake"][rank::2], g["c1_real"][rank::2][:700 - 300 * rank]
    return fake, real, m["imb8_model"][500 * rank:500 * rank + 400 + 100 * rank], m["imb8_centeroids"], float(m["imb8_thres"][0])


def _rank_states(rank):
    from cgs_amd.metrics import calibration_merge, calibration_state_of, mode_state_of
    fake, real, x, c, thres = _rank_inputs(rank)
    return calibration_merge(calibration_state_of(fake, 0), calibration_state_of(real, 1)), mode_state_of(x, c, thres)


def _gloo_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    from cgs_amd.metrics import all_reduce_calibration, all_reduce_modes
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cs, ms = _rank_states(rank)
    torch.save((all_reduce_calibration(cs), all_reduce_modes(ms)), out + f".{rank}")
    dist.destroy_process_group()


def test_all_reduce_over_gloo_equals_the_merge_of_the_two_host_states(tmp_path):
    import torch
    import torch.multiprocessing as mp
    from cgs_amd.metrics import calibration_merge, mode_merge
    out = str(tmp_path / "state")
    with socket.socket() as so:                                   # a free rendezvous port on the loopback interface
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, out), nprocs=2, join=True)
    (c0, m0), (c1, m1) = _rank_states(0), _rank_states(1)
    want_c, want_m = calibration_merge(c0, c1), mode_merge(m0, m1)
    assert want_c["label_max"][1] == max(c0["label_max"][1], c1["label_max"][1]) and want_c["n"] == 500 + 500 + 700 + 400
    for r in range(2):
        got_c, got_m = torch.load(out + f".{r}", weights_only=False)
        _same_state(got_c, want_c, tol=1e-15)
        assert np.array_equal(got_m["counts"], want_m["counts"]) and (got_m["n"], got_m["good"]) == (want_m["n"], want_m["good"]) == (900, want_m["good"])
        assert abs(got_m["sum_min"] - want_m["sum_min"]) <= 1e-15 * want_m["sum_min"]
