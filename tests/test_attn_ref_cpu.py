"""The CPU oracle's unfused attention chain against attn_ref over every case of attn_matrix, at the bars the device
is held to (attn_ref's docstring): proves the numpy reference, the chosen inputs and seeds, and the bars before a
GPU is involved.  attn_ref shares no code with the oracle, so where the two agree a restatement error of the
oracle's is ruled out.  Also: the planner fuses every graph case meant to fuse and refuses the refusals, the
`large` cases' scores are as large as declared, and a poison case's oracle output is its clean twin's."""
import numpy as np
import pytest

import attn_matrix as am
import attn_ref


def dead_rows_match(case, got, ref, orc):
    """A fully masked row: NaN exactly where the oracle has NaN."""
    if ref.dead.any():
        assert case.mask == "dead_row"
        assert np.array_equal(np.isnan(got[ref.dead]), np.isnan(orc[ref.dead])), f"{case.id}: NaN positions differ from the oracle's"


@pytest.mark.parametrize("case", am.CASES, ids=am.IDS)
def test_oracle_matches_attn_ref(case):
    ref = am.reference(case)
    orc, stats = am.oracle(case)
    assert ref.dead.any() == (case.mask == "dead_row")
    if case.rng == "large":
        print(f"{case.id}: max|w| {ref.wmax.max():.3f}")
        assert 20.0 <= ref.wmax.max() <= 30.0
    elif case.rng == "shift100":
        assert ref.wmax.min() > 89.0       # exp(89) is past f32
    else:
        assert ref.wmax.max() <= 8.0, f"{case.id}: an ordinary case with max|w| {ref.wmax.max():.2f}"
    attn_ref.check(f"{case.id} oracle vs attn_ref", orc, ref, case.bar)
    dead_rows_match(case, orc, ref, orc)
    if stats is not None:
        assert stats["attn"] == (1 if case.fuses else 0), (case.id, stats)
    if case.poison:
        clean, _ = am.oracle(am.twin(case))
        assert np.array_equal(orc.view(np.uint32), clean.view(np.uint32)), f"{case.id}: the oracle read past the window"


def test_large_bar_has_margin():
    """The worst |oracle - reference| of the `large` cases in units of 2^-24 (1 + max|w|) sum p|v|: twice it must
    still be within the derived C (attn_ref's docstring)."""
    worst = max(float(attn_ref.large_ratio(am.oracle(c)[0], am.reference(c)).max()) for c in am.CASES if c.rng == "large")
    print(f"large bar: worst oracle / reference ratio {worst:.4f}, C = {attn_ref.C_LARGE}")
    assert 2.0 * worst <= attn_ref.C_LARGE
