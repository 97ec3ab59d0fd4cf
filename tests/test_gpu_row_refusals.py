"""The device entry points against the table of row_refusal_cases.py: every mutation gives the code the host self test gives (both
run the same step function), a refusal sets hb_last_error where the entry point has a message and launches nothing, and the legal
set writes what the self test writes, bit for bit.  Operands are carved out of one device buffer."""
import numpy as np
import pytest

import row_refusal_cases as rc

pytestmark = pytest.mark.gpu

# A null operand is refused with the code alone, but by the demux steps, which fold it into their one text; every other refusal of the
# table carries the entry point's message.  The context keeps its last message, so before every mutation another entry point is made
# to refuse (nothing is launched): a message that begins with this entry point's name is then this call's.
def _has_message(step, change):
    return change[0] != "null" or step.family == "demux"


def _set_another_message(ctx, step):
    if step.entry != "hb_lt_leaves":
        rc_, name = ctx.lib.hb_lt_leaves(ctx.h, None, None, 0, 7, None, None, 0, None), b"hb_lt_leaves: "
    else:
        rc_, name = ctx.lib.hb_demux_mask(ctx.h, None, None, 0, 0, None, None, 0, None), b"hb_demux_mask: "
    assert rc_ == rc.BAD_ARG and ctx.lib.hb_last_error(ctx.h).startswith(name)


def _device_copy(ctx, buf):
    return ctx.torch.from_numpy(buf.copy()).to(ctx.tdev)


@pytest.mark.parametrize("p,nl", rc.FIELDS, ids=["wide", "narrow"])
def test_device_entry_points_refuse_what_the_self_tests_refuse(p, nl):
    import time

    from honeybadgermpc_amd._capi import Context

    ctx = Context.get(p)
    torch = ctx.torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wrong, calls = [], 0
    for step in rc.STEPS:
        # the legal set: HB_OK and the self test's outputs
        call = rc.Call(step, p, nl)
        host = call.buffer(sentinel=False)
        dev = _device_copy(ctx, host)
        consts = host.copy()
        assert call.selftest(host) == rc.OK, step.id
        got = call.device(ctx, dev.data_ptr(), consts.ctypes.data)
        torch.cuda.synchronize()
        if got != rc.OK or not np.array_equal(dev.cpu().numpy(), host):
            wrong.append((step.id, "legal", got))
        calls += 1
        for label, change, code in rc.mutations(step, p):
            call = rc.Call(step, p, nl, change)
            host = call.buffer()
            before = host.copy()
            dev = _device_copy(ctx, host)
            want = call.selftest(host)
            _set_another_message(ctx, step)
            got = call.device(ctx, dev.data_ptr(), before.ctypes.data)
            msg = ctx.lib.hb_last_error(ctx.h)
            torch.cuda.synchronize()
            after = dev.cpu().numpy()
            calls += 1
            if got != want or want != code:
                wrong.append((step.id, label, got, want, code))
            elif code == rc.BAD_ARG and not np.array_equal(after, before):
                wrong.append((step.id, label, "a refused call wrote"))
            elif code == rc.BAD_ARG and _has_message(step, change) and not (msg or b"").startswith(step.entry.encode() + b": "):
                wrong.append((step.id, label, "no message of this entry point", msg))
            elif code == rc.OK and not np.array_equal(after, host):
                wrong.append((step.id, label, "differs from the self test"))
    print("row refusals, %d limbs: %d calls in %.2f s" % (nl, calls, time.perf_counter() - t0))
    assert not wrong, wrong
