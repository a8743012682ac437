"""tts_hip_supports_op over the declared case list (ops_matrix): it answers 1 exactly for the nodes the generic op
kernels compute.  Host logic only; no device is opened and no case runs."""
import pytest

import ops_check
import ops_matrix


@pytest.mark.parametrize("case", ops_matrix.CASES, ids=lambda c: c.id)
def test_supports_op(case):
    g, outs = ops_check.build(case)
    want = int(case.expect == "run")
    for t in (outs if want else outs[-1:]):
        assert ops_check.supports(t) == want, f"{case.id}: supports_op says {1 - want}, the matrix expects {case.expect}"
    if want:    # every computed node of a run case (the chains' intermediates included) is one the kernels take
        for t in g.nodes:
            assert ops_check.supports(t) == 1, f"{case.id}: a node of a run case is refused"


def test_matrix_is_declared():
    """The run set and the refusal set are both there, and each run group is non-empty."""
    n_run = sum(c.expect == "run" for c in ops_matrix.CASES)
    n_ref = sum(c.expect == "refuse" for c in ops_matrix.CASES)
    assert n_run > 500 and n_ref > 80, (n_run, n_ref)
    assert all(c.expect in ("run", "refuse") and c.bar in ("bits", "ulp1") for c in ops_matrix.CASES)
    assert all(c.group == "refuse" for c in ops_matrix.CASES if c.expect == "refuse")
