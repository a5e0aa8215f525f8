"""The forward of the 2-D generator at 65..256 hidden units, host side: the two C ABI entries (csrc/mlp2d_wide_gen.hip), their refusals and
the workspace size.  The float64 reference of the GPU tests (test_gpu_synthetic_wide_gen.py) is the restatement of
test_synthetic_train_cpu.py, which is width-agnostic; it is checked here at 256 units against a direct numpy forward."""
import os
import re

import numpy as np
import pytest
import torch

import test_synthetic_train_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cgs_mlp2d_wide_gen_ws_bytes", "cgs_mlp2d_wide_gen_fwd")


def _fwd(l, nl, nh, B=1000, training=1, ws=None, ws_bytes=0):
    return l.cgs_mlp2d_wide_gen_fwd(None, None, None, None, None, None, nl, nh, None, None, B, training, 1e-5, None, ws, ws_bytes, None)


def test_new_symbols_are_declared_and_typed():
    from cgs_amd import lib
    header = open(os.path.join(ROOT, "include", "cgs_hip.h")).read()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        nargs = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs, name
    l = lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(l, name).argtypes == lib.SIGNATURES[name][1]
    # the same argument list as the narrow forward
    assert lib.SIGNATURES["cgs_mlp2d_wide_gen_fwd"] == lib.SIGNATURES["cgs_mlp2d_gen_fwd"]


@pytest.mark.parametrize("nl,nh", [(6, 64), (6, 257), (7, 256), (1, 256)])
def test_wide_forward_refuses_other_widths_and_depths(nl, nh):
    from cgs_amd import lib
    l = lib.load()
    assert _fwd(l, nl, nh) == lib.EINVAL and b"nlayers" in l.cgs_last_error()
    assert int(l.cgs_mlp2d_wide_gen_ws_bytes(1000, nl, nh)) == 0


@pytest.mark.parametrize("nl,nh", [(6, 256), (2, 65), (6, 128)])
def test_wide_forward_accepts_65_to_256_units(nl, nh):
    """Past the shape check the next refusal is the null weight array: still CGS_EINVAL, another message."""
    from cgs_amd import lib
    l = lib.load()
    assert _fwd(l, nl, nh) == lib.EINVAL and b"null weight array" in l.cgs_last_error()


def test_narrow_forward_still_stops_at_64_units():
    from cgs_amd import lib
    l = lib.load()
    rc = l.cgs_mlp2d_gen_fwd(None, None, None, None, None, None, 6, 256, None, None, 1000, 1, 1e-5, None, None, 0, None)
    assert rc == lib.EINVAL and b"nlayers" in l.cgs_last_error()


def test_wide_gen_workspace_size():
    """4 (nlayers-1) nhp (B + 2 ceil(B/32) + 2) bytes: every BN layer's pre-activations, the 32-row group partials, the (mean, rstd) rows."""
    from cgs_amd import lib
    l = lib.load()
    ws = lambda B, nl, nh: int(l.cgs_mlp2d_wide_gen_ws_bytes(B, nl, nh))
    assert ws(0, 6, 256) == 0 and ws(-1, 6, 256) == 0
    for nl, nh in ((6, 256), (2, 65), (4, 129), (6, 200)):
        nhp = (nh + 31) // 32 * 32
        last = 0
        for B in (1, 2, 31, 32, 33, 64, 65, 1000, 8200, 10000):
            got = ws(B, nl, nh)
            assert got == 4 * (nl - 1) * nhp * (B + 2 * ((B + 31) // 32) + 2)
            assert got >= (nl - 1) * B * nhp * 4 and got >= last and got > 0
            last = got


def test_restatement_is_width_agnostic():
    """g_forward at 256 x 6 in float64 against a direct numpy forward with batch statistics."""
    from cgs_amd.synthetic import MLPGenerator
    P = MLPGenerator.init_params(3, 256, 6)
    rs = np.random.RandomState(4)
    for k, v in P.items():
        if not k.endswith("/kernel"):
            P[k] = rs.uniform(0.5, 1.5, v.shape).astype(np.float32)
    z = rs.randn(50, 2)
    h = z
    for i in range(6):
        a = h @ P[f"generator/g_fc{i + 1}/kernel"].astype(np.float64) + P[f"generator/g_fc{i + 1}/bias"]
        if i == 5:
            break
        bn = R.bn_name(i)
        h = np.maximum((a - a.mean(0)) / np.sqrt(a.var(0) + R.EPS) * P[f"{bn}/gamma"] + P[f"{bn}/beta"], 0.0)
    got = R.g_forward(R.to_torch(P, torch.float64), torch.as_tensor(z), update=False).numpy()
    np.testing.assert_allclose(got, a, rtol=1e-12, atol=1e-12)
