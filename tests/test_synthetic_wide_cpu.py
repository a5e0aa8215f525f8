"""The width limits of the 2-D entry points, checked without a device: scoring and refining (cgs_mlp2d_sigmoid_saliency, cgs_refine2d,
cgs_refine2d_devbase) take 1..256 hidden units, what trains stays at 1..64.  Every call passes null weight arrays, so an accepted width
is refused by the NEXT check ("null weight") and nothing is launched."""
import pytest

ACCEPTED = ((6, 256), (2, 65), (6, 128))
REFUSED = ((6, 257), (6, 0), (7, 256))


def _calls(l, nl, nh):
    return {
        "cgs_mlp2d_sigmoid_saliency": lambda: l.cgs_mlp2d_sigmoid_saliency(None, None, nl, nh, None, None, None, 1000, 1e-3, None),
        "cgs_refine2d": lambda: l.cgs_refine2d(None, None, nl, nh, None, 0.5, 1e-3, 10, 0.1, 2, None, None, None, 1000, None),
        # the device-baseline form checks its baseline pointer first: give it a non-null one (never read: the width check comes next)
        "cgs_refine2d_devbase": lambda: l.cgs_refine2d_devbase(None, None, nl, nh, None, 4096, 1e-3, 10, 0.1, 2, None, None, None, 1000, None),
    }


@pytest.mark.parametrize("name", ["cgs_mlp2d_sigmoid_saliency", "cgs_refine2d", "cgs_refine2d_devbase"])
def test_scoring_and_refining_accept_up_to_256_units(name):
    from cgs_amd import lib
    l = lib.load()
    for nl, nh in ACCEPTED:
        rc = _calls(l, nl, nh)[name]()
        assert rc == lib.EINVAL and b"null weight" in l.cgs_last_error(), (nl, nh, l.cgs_last_error())
    for nl, nh in REFUSED:
        rc = _calls(l, nl, nh)[name]()
        msg = l.cgs_last_error()
        assert rc == lib.EINVAL and b"1..256" in msg and b"2..6" in msg and b"null" not in msg, (nl, nh, msg)


def test_d_step_still_stops_at_64_units():
    from cgs_amd import lib
    l = lib.load()
    rc = l.cgs_mlp2d_d_step(None, None, 6, 256, None, 1000, None, 1000, 1e-2, None, None, None, None, 0, None)
    assert rc == lib.EINVAL and b"1..64" in l.cgs_last_error(), l.cgs_last_error()
