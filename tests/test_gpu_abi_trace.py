"""What kernels.py hands to the C ABI, call by call, against tests/golden/abi_trace.json (tests/abi_trace_cases.py: the script, the
recorder and how a record is normalised).  Bar: equality.  The golden pins the order and the value of every argument of every entry
point the wrappers reach, every workspace byte count and which buffer carries it, every ``prepacked`` flag, which queries are asked,
and the keys and sums of the profile records.

The script runs in a process of its own: what a wrapper asks and packs depends on what ran before in the process, and the golden is
that of a fresh one.  After a change of the ABI that is meant, regenerate it on the device:
``python tests/abi_trace_cases.py tests/golden/abi_trace.json`` and review its diff."""
import json
import os
import subprocess
import sys

import pytest

import abi_trace_cases as AC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    out = tmp_path_factory.mktemp("abi_trace") / "trace.json"
    subprocess.run([sys.executable, os.path.join(AC.ROOT, "tests", "abi_trace_cases.py"), str(out)], check=True, timeout=300)
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    with open(AC.GOLDEN) as f:
        return json.load(f)


def test_trace_equals_the_golden(traced, golden):
    assert sorted(traced) == sorted(golden)
    for name in ("plain", "profiled"):
        assert len(traced[name]) == len(golden[name]), name
        for i, (got, want) in enumerate(zip(traced[name], golden[name])):
            assert got == want, f"{name} pass, call {i}"
    for name in ("profile", "profile_by_layer"):
        assert traced[name] == golden[name], name


def test_golden_names_every_entry_point_of_kernels_py(golden):
    seen = {r[0] for name in ("plain", "profiled") for r in golden[name]}
    assert not sorted(AC.kernels_source_names() - seen)


def test_second_run_is_the_first_with_the_weights_found_packed(traced):
    """The launches of the second pass are those of the first, argument for argument and buffer for buffer, except that every call with
    a packed-weight workspace now finds it packed."""
    from cgs_amd.lib import SIGNATURES
    first, second = ([r for r in traced[name] if AC.is_launch(r[0], SIGNATURES)] for name in ("plain", "profiled"))
    assert len(first) == len(second)
    packed_first = 0
    for a, b in zip(first, second):
        assert a[0] == b[0]
        want, at = list(a[1]), AC.prepacked_index(a[0], SIGNATURES)
        if at is not None and a[1][at - 2] is not None:
            packed_first += a[1][at] == 0
            want[at] = 1
        assert b[1] == want and b[2:] == a[2:], a[0]
    assert packed_first >= 9
