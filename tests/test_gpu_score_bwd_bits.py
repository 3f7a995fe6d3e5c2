"""The score backward's bits: tools/score_bwd_bits.py recomputes, for its fixed list of tiny problems (every bf16 form, the logQ and
bf16x3 forms, both fp8 forms, the hosted form), the SHA-256 of each direction's dA, and every case must equal the digest recorded in
tests/golden/score_bwd_bits.json -- written by the build its header names, never by the build under test.  A digest that differs
means an operation or its order changed in that case's kernel; a change that alters the arithmetic on purpose regenerates the file
and says so."""
import json
import sys

import pytest

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


def test_dA_bits_equal_the_recorded_build():
    golden = json.loads((GOLD / "score_bwd_bits.json").read_text())
    sys.path.insert(0, str(ROOT / "tools"))
    try:
        import score_bwd_bits
    finally:
        sys.path.pop(0)
    got = score_bwd_bits.digests()
    want = golden["cases"]
    assert sorted(got) == sorted(want), "the case list differs from the recorded one"
    differ = [case for case in want if got[case] != want[case]]
    print(f"{len(want)} cases against commit {golden['header']['commit']}: {len(differ)} differ")
    assert not differ, differ
