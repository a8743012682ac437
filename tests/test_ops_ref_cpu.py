"""The CPU oracle against ops_ref over every "run" case of ops_matrix, at the bars the device is held to
(ops_matrix's docstring): proves the numpy reference, the chosen inputs and the bars before a GPU is involved.
ops_ref shares no code with the oracle, so where the two agree a restatement error of the oracle's is ruled out."""
import pytest

import ops_check
import ops_matrix
import ops_ref


@pytest.mark.parametrize("group", ops_matrix.GROUPS)
def test_oracle_matches_ops_ref(group):
    for case in ops_matrix.by_group(group):
        if not case.oracle:
            continue
        g, outs = ops_check.build(case)
        ref = ops_ref.run(g)
        g.run_oracle()
        ops_check.check_against_ref(case, g, outs, ref)

