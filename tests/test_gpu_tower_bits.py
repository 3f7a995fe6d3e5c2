"""The tower passes' bits: tools/tower_bits.py recomputes, for its fixed list of tiny problems (every dispatch path of
tt_towers_mlp_fwd / _bwd's host code: front, narrow and wide tail, first-block backward, separate kernels, no hidden block, fp32,
eval, dropout, one tower alone, towers of different B, the SyncBN two-phase pass), the SHA-256 of each tower's unit rows, packed
images, dense gradients, d_x and BatchNorm running statistics, and every case must equal the digest recorded in
tests/golden/tower_bits.json -- written by the build its header names, never by the build under test.  A digest that differs means
a launch, one of its arguments or the arithmetic behind it changed on that path; a change that alters the arithmetic on purpose
regenerates the file and says so."""
import json
import sys

import pytest

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


def test_tower_pass_bits_equal_the_recorded_build():
    golden = json.loads((GOLD / "tower_bits.json").read_text())
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import tower_bits
    finally:
        sys.path.pop(0)
    got = tower_bits.digests()
    want = golden["cases"]
    assert sorted(got) == sorted(want), "the case list differs from the recorded one"
    differ = [case for case in want if got[case] != want[case]]
    print(f"{len(want)} cases against commit {golden['header']['commit']}: {len(differ)} differ")
    assert not differ, differ
