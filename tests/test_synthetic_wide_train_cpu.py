"""The argument checks of the wide D step (cgs_mlp2d_wide_d_step, cgs_mlp2d_wide_train_ws_bytes), without a device.  Every call passes
null weight arrays, so an accepted (nlayers, nhidden) is refused by the NEXT check ("null weight") and nothing is launched."""
import pytest

ACCEPTED = ((6, 256), (2, 65), (6, 128))
REFUSED = ((6, 257), (6, 64), (7, 256), (6, 0))


def _step(l, nl, nh):
    return l.cgs_mlp2d_wide_d_step(None, None, nl, nh, None, 1000, None, 1000, 1e-2, None, None, None, None, 0, None)


@pytest.mark.parametrize("nl,nh", ACCEPTED)
def test_wide_d_step_accepts_65_to_256_units(nl, nh):
    from cgs_amd import lib
    l = lib.load()
    rc = _step(l, nl, nh)
    assert rc == lib.EINVAL and b"null weight" in l.cgs_last_error(), (nl, nh, l.cgs_last_error())


@pytest.mark.parametrize("nl,nh", REFUSED)
def test_wide_d_step_refuses_other_widths_and_depths(nl, nh):
    from cgs_amd import lib
    l = lib.load()
    rc = _step(l, nl, nh)
    msg = l.cgs_last_error()
    assert rc == lib.EINVAL and b"65..256" in msg and b"2..6" in msg and b"null" not in msg, (nl, nh, msg)


def test_wide_train_workspace_size():
    from cgs_amd import lib
    ws = lib.load().cgs_mlp2d_wide_train_ws_bytes
    for bad in ((0, 6, 256), (-5, 6, 256), (2000, 1, 256), (2000, 7, 256), (2000, 6, 64), (2000, 6, 257), (2000, 6, 0), (2000, 0, 128)):
        assert ws(*bad) == 0, bad
    for nl, nh in ACCEPTED + ((3, 200), (2, 256)):
        last = 0
        # every batch around the sizes at which the chunk size of the weight-gradient pass changes (multiples of 2048), and large ones
        for Bt in list(range(1, 300)) + list(range(2040, 2060)) + list(range(4090, 4100)) + [20000, 20001, 100000]:
            n = ws(Bt, nl, nh)
            assert n > 0 and n >= last, (Bt, nl, nh, n, last)
            assert n >= 2 * Bt * (nl - 1) * nh * 4, (Bt, nl, nh, n)
            last = n
