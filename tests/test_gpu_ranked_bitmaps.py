"""k_ranked_stream (ranked_and with 3+ lists, and / and_freq with any number) asks a dense list's exact bitmap where it used to ask the
membership hint, and skips the weight round while a unit has no threshold (-m gpu). The case -- collection, queries, what is compared
-- is tests/ranked_bitmaps_probe.py; the reference (oracle scores, counts and freq sums, brute-force doc-id lists) is computed once
here, on the CPU, and every run below checks the same queries against it bit for bit in a fresh process, because the library reads
its knobs once per process: whole queries and queries split into units of 8 blocks (parts that share a floor: a threshold that forms
in another part), uploads without bitmaps (the hints answer, as before), finer tables (DS2I_RMW_G=2: other shifts, the other side of
the density rule) and 5+ lists left to the class kernels."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    import ranked_bitmaps_probe as probe
    path = str(tmp_path_factory.mktemp("ranked_bitmaps") / "reference.npz")
    probe.reference(path)
    return path


@pytest.mark.parametrize("knobs", ["", "DS2I_UNIT_CAP=8", "DS2I_NO_BITMAPS=1", "DS2I_NO_BITMAPS=1 DS2I_UNIT_CAP=8", "DS2I_RMW_G=2",
                                   "DS2I_RMW_G=2 DS2I_UNIT_CAP=8", "DS2I_STREAM_NT_MAX=4", "DS2I_STREAM_NT_MAX=4 DS2I_UNIT_CAP=8"])
def test_bitmaps_for_hints_bit_identical(built_lib, reference, knobs):
    env = dict(os.environ)
    for kn in knobs.split():
        name, val = kn.split("=")
        env[name] = val
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ranked_bitmaps_probe.py"), reference], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "ranked_bitmaps_probe ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
