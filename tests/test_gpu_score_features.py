"""RefineEngine.score_with_features: D's features from the scoring pass, against the oracle restatement of their definition -- D up to
(not including) its logit layer, batch statistics per logical batch, a map mean-pooled over space (what
tests/test_gpu_distribution.py::_features computes, with all 1024 coordinates for mnist) -- within 1e-4 of max|ref|, README's bar for
one forward evaluation.  The sigmoids are ``score``'s bit for bit; a refinement on the same engine is not disturbed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets_ref as N

CASES = [("mnist", 16, 1), ("dcgan32", 8, 2), ("cyclegan_tiny", 2, 1)]      # (arch, engine batch, bn_groups)
WIDTH = {"mnist": 1024, "dcgan32": 512, "cyclegan_tiny": 128}
_ORACLE = {}


def _oracle(arch, B, groups):
    """(params, images, features float64 [B, d]) -- computed once per arch, shared by the contraction modes."""
    if arch not in _ORACLE:
        P = N.init_params(arch, 2019, True)
        layers = N.ARCHS[arch]["d"]
        cut = max(i for i, L in enumerate(layers) if L[0] in ("linear", "conv"))
        body = [L for L in layers[:cut] if L[0] != "flatten"] if arch != "mnist" else layers[:cut]
        img = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, (B,) + tuple(N.ARCHS[arch]["img"])).astype(np.float32))
        b = B // groups
        feats = []
        with torch.no_grad():
            for i in range(0, B, b):
                f = N.run_layers(body, img[i:i + b], P, "discriminator", bn_training=True)
                feats.append(f.mean(dim=(1, 2)) if f.dim() == 4 else f)
        _ORACLE[arch] = (P, img, torch.cat(feats).double().numpy())
    return _ORACLE[arch]


@pytest.mark.parametrize("mode", ["f32", "bx6_all"])
@pytest.mark.parametrize("arch,B,groups", CASES)
def test_features_match_the_oracle_and_the_sigmoids_are_scores(arch, B, groups, mode):
    from cgs_amd.engine import RefineEngine
    from cgs_amd.nets import to_device
    d = torch.device("cuda:0")
    P, img, ref = _oracle(arch, B, groups)
    eng = RefineEngine(arch, to_device(P, d), B, d, bn_groups=groups, contraction=mode)
    assert eng.feature_width() == WIDTH[arch] == ref.shape[1]
    x = img.to(d)
    want_sig = eng.score(x).clone()
    sig, feat = eng.score_with_features(x)
    assert tuple(sig.shape) == (B, 1) and tuple(feat.shape) == (B, WIDTH[arch])
    assert torch.equal(sig, want_sig)
    err = np.abs(feat.cpu().double().numpy() - ref).max() / np.abs(ref).max()
    print(f"\n[score_with_features {arch} {mode}] max|delta| / max|ref| = {err:.3g} (bar 1e-4)")
    assert err < 1e-4
    # caller-owned outputs: the same values
    so, fo = torch.empty_like(sig), torch.full_like(feat, float("nan"))
    s2, f2 = eng.score_with_features(x, out=so, feat_out=fo)
    assert s2 is so and f2 is fo and torch.equal(so, want_sig) and torch.equal(fo, feat)


@pytest.mark.parametrize("arch,B,groups", CASES)
def test_a_following_refinement_is_what_it_is_without_the_features_call(arch, B, groups):
    from cgs_amd.engine import RefineEngine
    from cgs_amd.nets import to_device, g_input_shape, ARCHS
    d = torch.device("cuda:0")
    P, img, _ = _oracle(arch, B, groups)
    eng = RefineEngine(arch, to_device(P, d), B, d, bn_groups=groups)
    z = torch.from_numpy(np.random.RandomState(6).uniform(-1, 1, (B,) + g_input_shape(ARCHS[arch])).astype(np.float32)).to(d)
    before = [t.clone() for t in eng.refine_from_z(z, 2, 0.1)]
    eng.score_with_features(img.to(d))
    after = eng.refine_from_z(z, 2, 0.1)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
