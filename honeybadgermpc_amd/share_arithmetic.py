"""
Arithmetic on device share arrays (csrc/hb_ew.hip): what an MPC program does between its opens, on the (count, limbs)
int64 tensors that `Context.upload_ints`, `OpenCoalescer.open_share_array` and `offline.ShareDealer` speak.

Tensor level -- one launch each on torch's current stream, nothing synchronises unless it says so:

    add(ctx, a, b)   sub(ctx, a, b)   mul(ctx, a, b)   neg(ctx, a)        b: a tensor of a's length, or a Python int (broadcast)
    beaver_combine(ctx, d, e, p, q, pq)                                   d e + d q + e p + pq in one pass
    inv(ctx, a, check=True)                                               batched 1 / a; a zero raises ZeroDivisionError

(the local operators of the reference's ShareArray, progs/mixins/dataflow.py, and the list comprehensions of
progs/mixins/share_arithmetic.py:43 and :133).

Protocol level -- coroutines over an `OpenCoalescer`, tensors in and tensors out, mirroring the reference's mixins:

    beaver_multiply_arrays(co, x, y, (p, q, pq))             progs/mixins/share_arithmetic.py:24-45
    double_sharing_multiply_arrays(co, x, y, r_t, r_2t)      :71-103
    invert_share_array(co, xs, rs, mul_triples)              :120-135
    divide_share_arrays(co, xs, ys, rs, inv_triples, mul_triples)   :151-161

Preprocessing (triples, random shares, double sharings) is handed in as tensors: where it is stored is the caller's business.
Every party runs the same coroutine, so the opens meet batch for batch (see OpenCoalescer).  A result is computed on the
stream that is current when the opens have been delivered, behind the coalescer's own work on that stream.
"""
from ._capi import HB_EW_ADD, HB_EW_MUL, HB_EW_NEG, HB_EW_SUB


def _count(ctx, a, what):
    a = ctx.elems(a, what=what)
    return a, a.numel() // ctx.n_limbs


def _out(ctx, out, like, count):
    if out is None:
        return ctx.torch.empty_like(like)
    # Context.elems hands back a contiguous COPY of a strided tensor: fine for an input, useless for an output
    if isinstance(out, ctx.torch.Tensor) and not out.is_contiguous():
        raise ValueError("out: must be contiguous")
    return ctx.elems(out, count, what="out")


def _binary(ctx, op, name, a, b, out):
    a, count = _count(ctx, a, "a")
    broadcast = 0
    if op == HB_EW_NEG:
        b_ptr = None
    elif isinstance(b, int):
        b = ctx.upload_ints([b % ctx.modulus])
        b_ptr, broadcast = ctx.ptr(b), 1
    else:
        b = ctx.elems(b, count, what="b")
        b_ptr = ctx.ptr(b)
    out = _out(ctx, out, a, count)
    ctx.check(ctx.lib.hb_ew_op(ctx.h, op, ctx.ptr(a), b_ptr, broadcast, ctx.ptr(out), count, ctx.stream()), f"hb_ew_op({name})")
    return out


def add(ctx, a, b, out=None):
    """a + b element by element; b a tensor of a's length or a Python int added to every element.  out may be a or b."""
    return _binary(ctx, HB_EW_ADD, "add", a, b, out)


def sub(ctx, a, b, out=None):
    """a - b; b as in add"""
    return _binary(ctx, HB_EW_SUB, "sub", a, b, out)


def mul(ctx, a, b, out=None):
    """a * b; b a tensor (share times share: the degree doubles) or a Python int (a public scalar times a share array)"""
    return _binary(ctx, HB_EW_MUL, "mul", a, b, out)


def neg(ctx, a, out=None):
    """-a"""
    return _binary(ctx, HB_EW_NEG, "neg", a, None, out)


def beaver_combine(ctx, d, e, p, q, pq, out=None):
    """d e + d q + e p + pq (progs/mixins/share_arithmetic.py:43): d, e the opened x - p, y - q; (p, q, pq) this party's shares
    of the triples.  One fused launch: five reads and one write an element."""
    d, count = _count(ctx, d, "d")
    e, p, q, pq = (ctx.elems(v, count, what=w) for v, w in ((e, "e"), (p, "p"), (q, "q"), (pq, "pq")))
    out = _out(ctx, out, d, count)
    ctx.check(ctx.lib.hb_ew_beaver(ctx.h, ctx.ptr(d), ctx.ptr(e), ctx.ptr(p), ctx.ptr(q), ctx.ptr(pq), ctx.ptr(out), count, ctx.stream()),
              "hb_ew_beaver")
    return out


def inv(ctx, a, check=True, out=None):
    """1 / a element by element (batched: one field inversion per 8 or 16 elements).  check=True reads the kernel's zero counter
    back -- one synchronisation -- and raises ZeroDivisionError("Cannot invert zero") as field.py:126 does when the array held
    a zero.  check=False -> (inverses, counter): a one-element int32 tensor holding the number of zeros once the stream has
    got there; a zero's own output is 0 and the other inverses are right either way.  Nothing synchronises."""
    a, count = _count(ctx, a, "a")
    out = _out(ctx, out, a, count)
    zeros = ctx.torch.zeros(1, dtype=ctx.torch.int32, device=ctx.tdev)
    ctx.check(ctx.lib.hb_ew_inv(ctx.h, ctx.ptr(a), ctx.ptr(out), count, ctx.ptr(zeros), ctx.stream()), "hb_ew_inv")
    if not check:
        return out, zeros
    if int(zeros.item()):
        raise ZeroDivisionError("Cannot invert zero")
    return out


# ---- protocols over an OpenCoalescer -------------------------------------------------------------------------------
async def beaver_multiply_arrays(co, x, y, triples):
    """Shares of x[i] y[i] from shares x, y and one triple (p, q, pq) per element (BeaverMultiplyArrays,
    progs/mixins/share_arithmetic.py:24-45).  The two masked differences are queued before the first await: they travel as ONE
    coalesced batch."""
    ctx = co.ctx
    p, q, pq = triples
    f = co.open_share_array(sub(ctx, x, p))
    g = co.open_share_array(sub(ctx, y, q))
    d = await f
    e = await g
    return beaver_combine(ctx, d, e, p, q, pq)


async def double_sharing_multiply_arrays(co, x, y, r_t, r_2t):
    """Shares of x[i] y[i] by degree reduction (DoubleSharingMultiplyArrays, :71-103): the local products are a degree-2t
    sharing; masked by r_2t they are opened at degree 2t (n >= 3t + 1 parties, of which 2t + 1 honest columns must arrive) and
    the difference is added to r_t, the degree-t sharing of the same random values."""
    ctx = co.ctx
    xy_2t = mul(ctx, x, y)
    diff = await co.open_share_array(sub(ctx, xy_2t, r_2t, out=xy_2t), degree=2 * co.t)
    return add(ctx, r_t, diff)


async def invert_share_array(co, xs, rs, mul_triples):
    """Shares of 1 / x[i] (InvertShareArray, :120-135): sig = open(xs * rs) with one random share and one triple per element,
    every sig inverted in one batched launch, and rs scaled by the public 1 / sig -- a local product (the reference sends this
    second product through its share multiplication as well; a public factor needs no triple and no open).
    Raises ZeroDivisionError if an opened sig is zero (x[i] = 0, or r[i] = 0 with probability 1 / p)."""
    ctx = co.ctx
    sigs = await co.open_share_array(await beaver_multiply_arrays(co, xs, rs, mul_triples))
    return mul(ctx, rs, inv(ctx, sigs, check=True))


async def divide_share_arrays(co, xs, ys, rs, inv_triples, mul_triples):
    """Shares of x[i] / y[i] (DivideShareArrays, :151-161): ys inverted with (rs, inv_triples), then one more Beaver
    multiplication with mul_triples."""
    y_invs = await invert_share_array(co, ys, rs, inv_triples)
    return await beaver_multiply_arrays(co, xs, y_invs, mul_triples)
