"""
The MiMC block cipher on the device (csrc/hb_mimc.hip): the reference's progs/mimc.py (mimc_plain, mimc_mpc, mimc_mpc_batch) and
progs/mimc_symmetric.py (mimc_encrypt, mimc_decrypt), on the (count, limbs) int64 tensors the rest of the package speaks.

    F(x, k):  v = x;  for c in range(rounds): v = (v + k + c)^3;   F = v + k

    ROUND = 161                       the reference's constant for BLS12-381 Fr
    rounds_for(p)                     smallest R with 3**R >= p (integer arithmetic); rounds_for(BLS12-381 Fr) == ROUND
    mimc_plain(x, k, p, rounds)       host model on Python ints

Cleartext, one launch each on torch's current stream, nothing synchronises (322 dependent field multiplications an element over
BLS12-381, all in registers):

    mimc_plain_device(ctx, xs, key, rounds=None, out=None)           F(xs[i], key)
    mimc_keystream(ctx, key, count, start=0, rounds=None)            F(start + i, key), no input array
    mimc_encrypt(ctx, key, ms, start=0, rounds=None, out=None)       ms[i] + F(start + i, key)            (mimc_symmetric.py:10-16)
    mimc_decrypt_plain(ctx, key, cs, start=0, rounds=None, out=None) cs[i] - F(start + i, key): its inverse under a known key

Under MPC a round is x^3 = y^3 + 3 y^2 [r] + 3 y [r^2] + [r^3] with y = open(x - [r]) and one preprocessed cube ([r], [r^2], [r^3])
an element and round (progs/mimc.py:25-30, 46-55).  The next round's mask folds into the same pass, so a round is ONE open and ONE
launch and the round's share itself is never written:

    first_mask(ctx, xs, key, r0, start=0, out=None)                  xs + key - r0, the first array to open; xs None: the counters start + i
    cube_round(ctx, y, r, r2, r3, key, ctr, r_next=None, out=None)   x^3 + (key + ctr + 1) - r_next; r_next None (the last round): x^3 + key
    async mimc_mpc_batch(co, xs, key, cubes, rounds=None, start=0)   -> (count, limbs) shares of F(xs[i], key)
    async mimc_decrypt(co, key_share, cs, cubes, start=0, rounds=None)   -> shares of cs[i] - F(start + i, key)   (mimc_symmetric.py:19-28)

`key` is a Python int, or a tensor of one element (for all) or `count` elements.  Adding a public constant to a Shamir share is the
same addition on every party, so no function asks which of xs and key is the shared one: mimc_mpc_batch serves a shared x under a
public key, and a public x (xs None: counters) under a shared key, which is mimc_decrypt.  `cubes = (r, r2, r3)`, each
(rounds, count, limbs); round c uses row c.  Where preprocessing is stored is the caller's business.  rounds=None means
rounds_for(ctx.modulus).  Every party runs the same coroutine over its OpenCoalescer, so the opens meet batch for batch.
"""
from .._capi import HB_MIMC_PAIR, HB_MIMC_SUB
from ..share_arithmetic import _out, sub

BLS12_381 = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ROUND = 161


def rounds_for(p):
    """smallest R with 3**R >= p: ceil(log(p, 3)) of progs/mimc.py:7 without floating point"""
    if not isinstance(p, int) or p < 2:
        raise ValueError(f"p must be an integer above 1, got {p!r}")
    r, v = 0, 1
    while v < p:
        r, v = r + 1, 3 * v
    return r


def _rounds(p, rounds):
    if rounds is None:
        return rounds_for(p)
    if not isinstance(rounds, int) or isinstance(rounds, bool) or not 1 <= rounds < 1 << 31:
        raise ValueError(f"rounds must be an integer in [1, 2^31), got {rounds!r}")
    return rounds


def mimc_plain(x, k, p=BLS12_381, rounds=None):
    """F(x, k) on Python ints (mimc_plain of the reference for p = BLS12-381 Fr and rounds = ROUND)"""
    rounds = _rounds(p, rounds)
    v = x % p
    for ctr in range(rounds):
        v = pow(v + k + ctr, 3, p)
    return (v + k) % p


def _key(ctx, key, count):
    """-> (tensor, broadcast): an int or a one-element tensor serves every element"""
    if isinstance(key, int) and not isinstance(key, bool):
        return ctx.upload_ints([key % ctx.modulus]), 1
    key = ctx.elems(key, what="key")
    have = key.numel() // ctx.n_limbs
    if have == 1:
        return key, 1
    if have != count:
        raise ValueError(f"key: expected 1 or {count} elements, got {have}")
    return key, 0


def _start(ctx, start):
    if not isinstance(start, int) or isinstance(start, bool):
        raise TypeError(f"start: expected an int, got {type(start).__name__}")
    return ctx.host_elems([start % ctx.modulus])


def _plain(ctx, xs, count, start, key, addend, flags, rounds, out, pair):
    rounds = _rounds(ctx.modulus, rounds)
    key, broadcast = _key(ctx, key, count)
    start = _start(ctx, start)
    out = ctx.empty(count) if out is None else _out(ctx, out, None, count)
    if broadcast and count > 1 and out.data_ptr() == key.data_ptr():
        raise ValueError("out: must not be the key that serves every element")
    ctx.check(ctx.lib.hb_mimc_plain(ctx.h, None if xs is None else ctx.ptr(xs), start.ctypes.data, ctx.ptr(key), broadcast,
                                    None if addend is None else ctx.ptr(addend), flags | (HB_MIMC_PAIR if pair else 0), rounds, ctx.ptr(out), count,
                                    ctx.stream()), "hb_mimc_plain")
    return out


def _count(count):
    if not isinstance(count, int) or isinstance(count, bool) or count < 0:
        raise ValueError(f"count must be a non-negative integer, got {count!r}")
    return count


def mimc_plain_device(ctx, xs, key, rounds=None, out=None, pair=False):
    """F(xs[i], key) in one launch.  out may be xs.  pair=True: two elements a thread (same results)."""
    xs = ctx.elems(xs, what="xs")
    return _plain(ctx, xs, xs.numel() // ctx.n_limbs, 0, key, None, 0, rounds, out, pair)


def mimc_keystream(ctx, key, count, start=0, rounds=None, pair=False):
    """F(start + i, key) for i < count: the counters are made in the kernel, nothing is read but the key"""
    return _plain(ctx, None, _count(count), start, key, None, 0, rounds, None, pair)


def mimc_encrypt(ctx, key, ms, start=0, rounds=None, out=None, pair=False):
    """ms[i] + F(start + i, key) (mimc_encrypt, progs/mimc_symmetric.py:10-16, whose counters start at 0).  out may be ms."""
    ms = ctx.elems(ms, what="ms")
    return _plain(ctx, None, ms.numel() // ctx.n_limbs, start, key, ms, 0, rounds, out, pair)


def mimc_decrypt_plain(ctx, key, cs, start=0, rounds=None, out=None, pair=False):
    """cs[i] - F(start + i, key): what mimc_encrypt added, taken off again by a holder of the key.  out may be cs."""
    cs = ctx.elems(cs, what="cs")
    return _plain(ctx, None, cs.numel() // ctx.n_limbs, start, key, cs, HB_MIMC_SUB, rounds, out, pair)


def first_mask(ctx, xs, key, r0, start=0, out=None):
    """xs + key - r0: the array the first round opens.  xs None: the counters start + i (public blocks under a shared key).
    One launch; out may be xs or r0."""
    r0 = ctx.elems(r0, what="r0")
    count = r0.numel() // ctx.n_limbs
    if xs is not None:
        xs = ctx.elems(xs, count, what="xs")
    key, broadcast = _key(ctx, key, count)
    start = _start(ctx, start)
    out = ctx.empty(count) if out is None else _out(ctx, out, None, count)
    if broadcast and count > 1 and out.data_ptr() == key.data_ptr():
        raise ValueError("out: must not be the key that serves every element")
    ctx.check(ctx.lib.hb_mimc_first(ctx.h, None if xs is None else ctx.ptr(xs), start.ctypes.data, ctx.ptr(key), broadcast, ctx.ptr(r0), ctx.ptr(out), count,
                                    ctx.stream()), "hb_mimc_first")
    return out


def cube_round(ctx, y, r, r2, r3, key, ctr, r_next=None, out=None):
    """After the open of round ctr: y the opened x - r, (r, r2, r3) this party's shares of the round's cube.
    x^3 = y^3 + 3 y^2 r + 3 y r2 + r3; -> x^3 + (key + ctr + 1) - r_next, the next round's array to open, or, with r_next None
    (the last round), x^3 + key.  One fused launch: five reads and one write an element.  out may be any of the arrays."""
    if not isinstance(ctr, int) or isinstance(ctr, bool) or not 0 <= ctr < (1 << 63) - 1:
        raise ValueError(f"ctr must be an integer in [0, 2^63 - 1), got {ctr!r}")
    y = ctx.elems(y, what="y")
    count = y.numel() // ctx.n_limbs
    r, r2, r3 = (ctx.elems(v, count, what=w) for v, w in ((r, "r"), (r2, "r2"), (r3, "r3")))
    if r_next is not None:
        r_next = ctx.elems(r_next, count, what="r_next")
    key, broadcast = _key(ctx, key, count)
    out = ctx.empty(count) if out is None else _out(ctx, out, None, count)
    if broadcast and count > 1 and out.data_ptr() == key.data_ptr():
        raise ValueError("out: must not be the key that serves every element")
    ctx.check(ctx.lib.hb_mimc_round(ctx.h, ctx.ptr(y), ctx.ptr(r), ctx.ptr(r2), ctx.ptr(r3), ctx.ptr(key), broadcast, ctr,
                                    None if r_next is None else ctx.ptr(r_next), ctx.ptr(out), count, ctx.stream()), "hb_mimc_round")
    return out


def _cubes(ctx, cubes, rounds, count=None):
    t = ctx.torch
    try:
        r, r2, r3 = cubes
    except (TypeError, ValueError):
        raise ValueError("cubes: expected (r, r2, r3)") from None
    rows = []
    for v, w in ((r, "cubes r"), (r2, "cubes r2"), (r3, "cubes r3")):
        if not isinstance(v, t.Tensor) or v.dim() != 3 or v.shape[2] != ctx.n_limbs or (count is not None and v.shape[1] != count):
            raise ValueError(f"{w}: expected a tensor of shape (rounds, {'count' if count is None else count}, {ctx.n_limbs})")
        if count is None:
            count = v.shape[1]
        if v.shape[0] < rounds:
            raise ValueError(f"{w}: {rounds} rounds take {rounds} rows, got {v.shape[0]}")
        rows.append(ctx.elems(v, what=w))
    return rows, count


async def mimc_mpc_batch(co, xs, key, cubes, rounds=None, start=0):
    """Shares of F(xs[i], key) (mimc_mpc_batch, progs/mimc.py:40-64; with a key per element or xs None also the gathered mimc_mpc
    calls of mimc_decrypt): first_mask, then `rounds` times one coalesced open and one cube_round.  xs None: the public counters
    start + i, as many as the cubes have columns.  xs and the cubes are left untouched; the rounds ping-pong between two buffers."""
    ctx = co.ctx
    rounds = _rounds(ctx.modulus, rounds)
    count = None
    if xs is not None:
        xs = ctx.elems(xs, what="xs")
        count = xs.numel() // ctx.n_limbs
    (r, r2, r3), count = _cubes(ctx, cubes, rounds, count)
    key, _ = _key(ctx, key, count)                      # an int is uploaded once, not once a round
    buffers = [ctx.empty(count), ctx.empty(count)]
    cur = first_mask(ctx, xs, key, r[0], start=start, out=buffers[1])
    for c in range(rounds):
        y = await co.open_share_array(cur)
        cur = cube_round(ctx, y, r[c], r2[c], r3[c], key, c, r_next=r[c + 1] if c + 1 < rounds else None, out=buffers[c & 1])
    return cur


async def mimc_decrypt(co, key_share, cs, cubes, start=0, rounds=None):
    """Shares of cs[i] - F(start + i, key) from a share of the key and the public ciphertexts (mimc_decrypt,
    progs/mimc_symmetric.py:19-28): the keystream blocks are evaluated together, one open a round for all of them."""
    ctx = co.ctx
    cs = ctx.elems(cs, what="cs")
    _cubes(ctx, cubes, _rounds(ctx.modulus, rounds), cs.numel() // ctx.n_limbs)       # one column of cubes a ciphertext block
    stream = await mimc_mpc_batch(co, None, key_share, cubes, rounds=rounds, start=start)
    return sub(ctx, cs, stream, out=stream)
