"""The generic op kernels (k_ops.hip) over the declared case list (ops_matrix): strided, typed and edge-valued
forms of every op tts_hip_supports_op says yes to, each "run" case as its own graph on the device, compared with

  ops_ref   (numpy, shares nothing with the kernels) at the case's bar: bit equality for moves and the singly
            rounded ops; at most 1 ulp with >= 99.9 % of the elements bit-equal for the transcendental ops and
            the reductions -- and not one byte outside the output's elements changed;
  the oracle, bit for bit, the project's standing bar.

A "refuse" case is never executed: supports_op is asserted to refuse it, and is asserted to accept every run
case here as well, so no case leaves the run set by being refused.
"""
import pytest

import ops_check
import ops_matrix
import ops_ref


@pytest.mark.gpu
@pytest.mark.parametrize("group", ops_matrix.GROUPS)
def test_ops_strided(hip, group):
    cases = ops_matrix.by_group(group)
    assert cases and all(c.expect == "run" for c in cases)
    for case in cases:
        g, outs = ops_check.build(case)
        for t in g.nodes:
            assert ops_check.supports(t) == 1, f"{case.id}: a node of a run case is refused"
        ref = ops_ref.run(g)
        g.run_hip(hip)
        ops_check.check_against_ref(case, g, outs, ref)
        if case.oracle:
            go, oo = ops_check.build(case)
            go.run_oracle()
            for k, (a, b) in enumerate(zip(outs, oo)):
                ops_check.compare(f"{case.id}[{k}] vs oracle", ops_ref.read(g, g.arrays, a), ops_ref.read(go, go.arrays, b), "bits")


@pytest.mark.gpu
def test_refusals_stay_off_the_device(hip):
    refused = ops_matrix.by_group("refuse")
    assert refused and all(c.expect == "refuse" for c in refused)
    for case in refused:
        g, outs = ops_check.build(case)
        assert ops_check.supports(outs[-1]) == 0, f"{case.id}: accepted"
