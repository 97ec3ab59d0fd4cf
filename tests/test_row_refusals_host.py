"""The host self tests refuse what the device entry points refuse: both run the step functions of csrc/hb_rows.hpp, so an output laid
over an input, a shape parameter past its bound or a missing operand is HB_ERR_BAD_ARG with nothing written -- on the host, with no
GPU.  The table is row_refusal_cases.py; test_gpu_row_refusals.py holds the device entry points to the same codes."""
import numpy as np
import pytest

import row_refusal_cases as rc

CASES = [pytest.param(step, p, nl, id="%s-%d" % (step.id, nl)) for step in rc.STEPS for p, nl in rc.FIELDS]


@pytest.mark.parametrize("step,p,nl", CASES)
def test_legal_set_is_accepted_and_equals_the_existing_driver(step, p, nl):
    call = rc.Call(step, p, nl)
    buf = call.buffer(sentinel=False)
    before = buf.copy()
    assert call.selftest(buf) == rc.OK
    want = rc.driver_outputs(call)
    for o in step.outs:
        assert call.output(buf, o.name).tobytes() == want[o.name], o.name
    # nothing but the outputs is written
    for o in step.outs:
        call.output(buf, o.name)[:] = call.output(before, o.name)
    assert np.array_equal(buf, before)


@pytest.mark.parametrize("step,p,nl", CASES)
def test_every_mutation_gives_its_code_and_a_refusal_writes_nothing(step, p, nl):
    wrong = []
    for label, change, code in rc.mutations(step, p):
        call = rc.Call(step, p, nl, change)
        buf = call.buffer()
        before = buf.copy()
        got = call.selftest(buf)
        if got != code or (code == rc.BAD_ARG and not np.array_equal(buf, before)):
            wrong.append((label, got, code, "written" if not np.array_equal(buf, before) else "untouched"))
    assert not wrong, wrong


def test_the_table_has_every_mutation_kind_for_every_step():
    for step in rc.STEPS:
        kinds = {change[0] for _, change, _ in rc.mutations(step, rc.WIDE)}
        assert "null" in kinds
        assert ("over" in kinds) == step.apart, step.id
