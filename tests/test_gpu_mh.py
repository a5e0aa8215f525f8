"""csrc/mh.hip on the device against the numpy fp32 statement of tests/mh_cases.py.

walk.  Bar: equality, with no tolerance -- rows, counts, span, the state (d and cnt) and fill are those of the statement, which
test_mh_cases_cpu holds to the host ``IndependenceSampler.walk`` on every case.  Each case is two calls, the second continuing the chain
of the first as two host calls do, and a rerun of both from the same start, which has to be bit-equal.  Sizes: b = 1, 2, 63 / 64 / 65 (a
window), 129 (two windows and one row), 1000; 1 / 3 / 32 segments; one segment of 10 000 and one of 50 000 constant scores (every
proposal moves: the longest serial path); take_all on the first, a middle, the last and every segment; the pool filled inside a segment,
exactly at a segment end, before the call and by the call before.

gather.  Bar: bit equality with src[rows] at span[0] on, every other row of dst untouched: repeated rows, row lengths 1, 2, 3, 63, 75
(4-byte pieces), 784 (196 16-byte pieces), bases off by one float (the scalar branch of a row length that would allow 16 bytes),
clipping at the pool's end, an index outside the source, and span[1] = 0."""
import numpy as np
import pytest
import torch

import mh_cases as MC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: the cached inputs are read-only)


def _sampler(case):
    from cgs_amd.sampling import DeviceIndependenceSampler
    s = DeviceIndependenceSampler(T=case["T"], B=case["B"], device=DEV)
    s.set_score_curr(case["seed"])
    s.cnt_chain = case["cnt0"]
    assert s.d_curr == float(case["seed"]) and s.cnt_chain == case["cnt0"]
    return s


def _run(case):
    s = _sampler(case)
    fill = torch.full((1,), case["fill0"], dtype=torch.int64, device=DEV) if case["capacity"] is not None else None
    out = []
    for call in case["calls"]:
        rows, counts, span = s.walk_device(_dev(call["sig"]), call["u"], case["groups"], call["take_all"], fill, case["capacity"])
        span = span.cpu().numpy()
        out.append(dict(rows=rows.cpu().numpy()[:int(span[1])], counts=counts.cpu().numpy(), span=span, d=s.d_curr, cnt=s.cnt_chain,
                        fill=int(fill.cpu()[0]) if fill is not None else None))
    return out


@pytest.mark.parametrize("name", MC.case_names())
def test_walk_equals_the_statement(name):
    case = MC.build(name)
    first, again = _run(case), _run(case)
    for call, got, rerun in zip(case["calls"], first, again):
        ref = call["ref"]
        assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], ref["counts"])
        assert got["span"].dtype == np.int64 and got["span"].tolist() == [ref["span"][0] if case["capacity"] is not None else 0, ref["span"][1]]
        assert got["rows"].dtype == np.int32 and np.array_equal(got["rows"], ref["rows"])
        assert got["d"] == ref["d"] and got["cnt"] == ref["cnt"]
        if case["capacity"] is not None:
            assert got["fill"] == ref["fill"]
        for k in ("rows", "counts", "span"):                             # a rerun from the same start: bit-equal
            assert np.array_equal(rerun[k], got[k])
        assert rerun["d"] == got["d"] and rerun["cnt"] == got["cnt"] and rerun["fill"] == got["fill"]


def test_read_back_walk_and_drawn_uniforms_follow_the_host_class():
    """``walk`` reads rows and counts back; without uniforms the class draws them as the host class consumes the stream: b per walked
    segment, none for a segment taken whole."""
    from cgs_amd.sampling import IndependenceSampler
    case = MC.build("take-middle")
    call, b = case["calls"][0], case["b"]
    s = _sampler(case)
    np.random.seed(5)
    rows, counts = s.walk(_dev(call["sig"]).reshape(-1, 1), None, case["groups"], call["take_all"])
    after = np.random.uniform(0, 1, size=3)
    h = IndependenceSampler(T=case["T"], B=case["B"])
    h.set_score_curr(case["seed"])
    h.cnt_chain = case["cnt0"]
    np.random.seed(5)
    want = []
    for g in range(case["groups"]):
        got = list(range(b)) if call["take_all"][g] else h.walk(call["sig"][g * b:(g + 1) * b].reshape(b, 1).copy())
        want.append([g * b + r for r in got])
    assert np.array_equal(np.random.uniform(0, 1, size=3), after)
    assert rows.tolist() == sum(want, []) and counts.tolist() == [len(w) for w in want]
    assert s.d_curr == float(np.ravel(h.d_curr)[0]) and s.cnt_chain == h.cnt_chain
    s.set_score_curr(torch.full((1,), 0.3137, dtype=torch.float32, device=DEV))                # a device seed
    assert s.d_curr == float(np.float32(0.3137))


# ---------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("row", [1, 2, 3, 63, 75, 784, 1024, 1028])     # 1024: 256 float4 pieces, a block; 1028: 257, the first row that spans two
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off-by-one-float"])
def test_gather_rows(row, off):
    from cgs_amd import kernels as K
    rs = np.random.RandomState(row + off)
    n, cap = 37, 50
    src = rs.randn(n, row).astype(np.float32)
    src_d = _dev(np.concatenate([np.zeros(off, np.float32), src.reshape(-1)]))[off:].reshape(n, row)      # the base moved by `off` floats
    assert src_d.data_ptr() % 16 == 4 * off
    picks = rs.randint(n, size=n).astype(np.int32)
    picks[3] = picks[4] = picks[5] = picks[30]                         # repeats
    picks[7], picks[8] = -1, n                                          # outside the source: nothing copied
    for at, listed in ((0, n), (5, 20), (30, 37), (49, 5), (50, 3), (12, 0)):
        back = rs.randn(cap * row + off).astype(np.float32)
        dst_flat = _dev(back)
        dst = dst_flat[off:].reshape(cap, row)
        K.gather_rows(src_d, _dev(picks), _dev(np.asarray([at, listed], dtype=np.int64)), dst)
        want = back[off:].reshape(cap, row).copy()
        for k in range(listed):
            if at + k < cap and 0 <= picks[k] < n:
                want[at + k] = src[picks[k]]
        got = dst_flat.cpu().numpy()
        assert np.array_equal(got[off:].reshape(cap, row), want), (at, listed)
        assert np.array_equal(got[:off], back[:off])


def test_gather_after_a_walk_fills_a_pool_like_the_host_loop():
    """Walk, then gather images, through the class: the pool rows are batch[rows], appended at the fill count, cut at the pool's end."""
    case = MC.build("full-inside")
    call = case["calls"][0]
    n = case["b"] * case["groups"]
    s = _sampler(case)
    imgs = np.random.RandomState(2).randn(n, 7, 7, 3).astype(np.float32)
    pool = torch.full((case["capacity"], 7, 7, 3), -5.0, device=DEV)
    fill = torch.zeros(1, dtype=torch.int64, device=DEV)
    rows, counts, span = s.walk_device(_dev(call["sig"]), call["u"], case["groups"], None, fill, case["capacity"])
    s.gather(_dev(imgs), pool, span, rows)
    assert np.array_equal(pool.cpu().numpy(), imgs[call["ref"]["rows"]][:case["capacity"]])
    assert int(fill.cpu()[0]) == call["ref"]["fill"] > case["capacity"]


def test_bad_arguments_are_refused_without_a_launch():
    from cgs_amd import kernels as K
    from cgs_amd import lib as L
    sig = torch.rand(6, device=DEV)
    u = torch.rand(6, dtype=torch.float64, device=DEV)
    st = torch.tensor([0.5, 1.0], dtype=torch.float64, device=DEV)
    keep = st.clone()
    with pytest.raises(L.CgsError):
        K.mh_walk(sig, u[:5], st, 5)                                     # one uniform short
    with pytest.raises(L.CgsError):
        K.mh_walk(sig, u, st, 5, groups=4)                               # no whole batches
    with pytest.raises(L.CgsError):
        K.mh_walk(sig, u, st, -1)
    with pytest.raises(L.CgsError):
        K.mh_walk(sig, u, st, 5, B=-1)
    with pytest.raises(L.CgsError):
        K.mh_walk(sig, u, st[:1], 5)                                     # the state is two doubles
    with pytest.raises(L.CgsError):
        K.mh_walk(sig.double(), u, st, 5)
    with pytest.raises(L.CgsError):
        K.mh_walk(sig, u, st, 5, fill=torch.zeros(1, dtype=torch.int64, device=DEV))          # fill without capacity
    with pytest.raises(L.CgsError):
        K.mh_walk(sig, u, st, 5, fill=torch.zeros(1, dtype=torch.int64, device=DEV), capacity=-1)
    with pytest.raises(L.CgsError):
        K.mh_walk(sig, u, st, 5, groups=2, take_all=torch.zeros(3, dtype=torch.uint8, device=DEV))
    rows, span = torch.zeros(6, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    x = torch.rand(6, 2, device=DEV)
    with pytest.raises(L.CgsError):
        K.gather_rows(x, rows, span, torch.zeros((4, 3), device=DEV))    # rows of another length
    with pytest.raises(L.CgsError):
        K.gather_rows(x, rows.long(), span, torch.zeros((4, 2), device=DEV))
    with pytest.raises(L.CgsError):
        K.gather_rows(x, rows, span[:1], torch.zeros((4, 2), device=DEV))
    l = L.load()
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    cnt, sp, fl = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    args = lambda b, nbytes: (sig.data_ptr(), b, 1, u.data_ptr(), 5, 0, None, st.data_ptr(), fl.data_ptr(), 10, rows.data_ptr(), cnt.data_ptr(), sp.data_ptr(),
                              ws.data_ptr(), nbytes, None)
    assert l.cgs_mh_walk(*args(6, 16)) == L.EWORKSPACE                   # 6 ints need 24 bytes
    assert l.cgs_mh_walk(*args(0, 512)) == L.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(st, keep) and int(fl.cpu()[0]) == 0              # nothing ran
