"""
Public-key encryption towards the MPC system (the reference's progs/mimc_jubjub_pkc.py) on device tensors: the key pair is a bitwise
shared x and the opened point [x] GP; a client derives k = (a pub_key).x, sends a GP along and runs MiMC in counter mode; the system
computes [k] = ([x] (a GP)).x from its bit shares and decrypts under the shared key.

    GP                                                              the generator the reference hard-codes (:9-11), order 8 r_J
    async key_generation(co, bits, triples, rs)                     -> (bits, pub_key Point): share_mul on GP, both coordinates opened
                                                                    in one batch.  The bit shares (K, 1, limbs) are handed in, as all
                                                                    preprocessing is here (the reference draws them, :21)
    mimc_encrypt(ctx, pub_key, ms, a)                               -> (ciphertext tensor, a_): `a` is required (the reference's seed).
                                                                    One client: a an int, ms (blocks, limbs) -> a_ a host Point (this
                                                                    synchronises, to hand the point back).  Many clients: a a tensor of
                                                                    B scalars, ms (B, blocks, limbs), client i under its own key ->
                                                                    ciphertext (B, blocks, limbs), a_ a tensor pair of B points; nothing
                                                                    synchronises.
    async mimc_decrypt(co, bits, (cs, a_), add_triples, add_rs, cubes)   -> shares of the messages, shaped as cs.  One client: bits
                                                                    (K, 1, limbs), a_ a Point, cs (blocks, limbs).  B clients: bits
                                                                    (K, B, limbs), a_ a tensor pair, cs (B, blocks, limbs): one key share
                                                                    a client (a key per element of the cipher).  add_triples / add_rs
                                                                    as share_mul takes them ((K - 1) B pairs), cubes as
                                                                    progs.mimc.mimc_decrypt takes them (161 rows of B blocks columns).
"""
from ..elliptic_curve import Point
from ..share_arithmetic import add, sub
from . import jubjub, mimc

GP = Point(5, 6846412461894745224441235558443359243034138132682534265960483512729196124138)


async def key_generation(co, bits, triples, rs):
    """-> (bits, pub_key): pub_key = open([x] GP) as a host Point, x = sum bits[j] 2^j (key_generation, :14-26)"""
    ctx = co.ctx
    if not isinstance(bits, ctx.torch.Tensor) or bits.dim() != 3 or bits.shape[1] != 1:
        raise ValueError("bits: one key pair takes bit shares of shape (K, 1, limbs)")
    xs, ys = await jubjub.share_mul(co, bits, GP, triples, rs)
    fx, fy = co.open_share_array(xs), co.open_share_array(ys)
    x, y = await fx, await fy
    return bits, Point(ctx.download_ints(x)[0], ctx.download_ints(y)[0], GP.curve)


def mimc_encrypt(ctx, pub_key, ms, a):
    """counter-mode MiMC under k = (a pub_key).x, with a_ = a GP for the decryption (mimc_encrypt, :29-54)"""
    t = ctx.torch
    if not isinstance(pub_key, Point):
        raise TypeError(f"pub_key: expected a Point, got {type(pub_key).__name__}")
    if isinstance(a, int) and not isinstance(a, bool):
        ms = ctx.elems(ms, what="ms")
        ax, ay = jubjub.scalar_mul(ctx, a, GP)
        kx, _ = jubjub.scalar_mul(ctx, a, pub_key)
        cs = mimc.mimc_encrypt(ctx, kx, ms)
        return cs, Point(ctx.download_ints(ax)[0], ctx.download_ints(ay)[0], GP.curve)
    a = ctx.elems(a, what="a")
    clients = a.numel() // ctx.n_limbs
    if not isinstance(ms, t.Tensor) or ms.dim() != 3 or ms.shape[0] != clients:
        raise ValueError(f"ms: {clients} clients take a tensor of shape ({clients}, blocks, {ctx.n_limbs})")
    blocks = int(ms.shape[1])
    ms = ctx.elems(ms, clients * blocks, what="ms")
    a_ = jubjub.scalar_mul(ctx, a, GP)
    kx, _ = jubjub.scalar_mul(ctx, a, pub_key)
    keys, counters = _per_block(ctx, kx, clients, blocks)
    stream = mimc.mimc_plain_device(ctx, counters, keys)
    return add(ctx, ms, stream, out=stream).reshape(clients, blocks, ctx.n_limbs), a_


def _per_block(ctx, keys, clients, blocks):
    """-> (keys, counters), each (clients * blocks, limbs): element (i, j) is block j of client i, its counter j, its key client i's"""
    shape = (clients, blocks, ctx.n_limbs)
    keys = keys.reshape(clients, 1, ctx.n_limbs).expand(*shape).reshape(clients * blocks, ctx.n_limbs)
    counters = ctx.upload_ints(list(range(blocks))).reshape(1, blocks, ctx.n_limbs).expand(*shape).reshape(clients * blocks, ctx.n_limbs)
    return keys, counters


async def mimc_decrypt(co, bits, ciphertext, add_triples, add_rs, cubes):
    """shares of the messages from the bit shares of the private key (mimc_decrypt, :57-79): [k] = ([x] a_).x by share_mul, then the
    keystream under the shared key, one open a round for every block of every client"""
    ctx = co.ctx
    t = ctx.torch
    cs, a_ = ciphertext
    kx, _ = await jubjub.share_mul(co, bits, a_, add_triples, add_rs)
    clients = kx.shape[0]
    if clients == 1 and cs.dim() == 2:
        return await mimc.mimc_decrypt(co, kx, cs, cubes)
    if not isinstance(cs, t.Tensor) or cs.dim() != 3 or cs.shape[0] != clients:
        raise ValueError(f"cs: {clients} clients take a tensor of shape ({clients}, blocks, {ctx.n_limbs})")
    blocks = int(cs.shape[1])
    flat = ctx.elems(cs, clients * blocks, what="cs")
    keys, counters = _per_block(ctx, kx, clients, blocks)
    stream = await mimc.mimc_mpc_batch(co, counters, keys, cubes)
    return sub(ctx, flat, stream, out=stream).reshape(clients, blocks, ctx.n_limbs)
