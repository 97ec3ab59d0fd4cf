"""
The iterated butterfly (switching) network on the device (csrc/hb_bf.hip): the mixer the reference's AsynchroMix server runs
(apps/asynchromix/butterfly_network.py:9-53, called from apps/asynchromix/asynchromix.py:383), on the (count, limbs) int64
tensors the rest of the package speaks.

k inputs, k a power of two, go through log2(k)^2 layers: log2(k) iterations of the strides 1, 2, 4, ..., k / 2.  A layer with
stride s = 2^a has k / 2 switches; switch j takes

    x = in[xi],  y = in[yi],    xi = ((j >> a) << (a + 1)) | (j & (s - 1)),   yi = xi | s

a shared random sign b_j in {1, -1} and one Beaver triple, and computes m = b_j (x - y),

    out[2j] = (x + y + m) / 2,   out[2j + 1] = (x + y - m) / 2

so b = 1 passes the pair straight and b = -1 crosses it.  The multiplication opens b_j - p_j and (x - y) - q_j: a layer is two
fused launches around one open.

    layers(k)                         -> [log2_stride, ...] of length log2(k)^2, in the reference's order
    switch_indices(k, log2_stride)    -> (xi, yi) as lists of ints: the host model of the wiring
    permutation(k, signs)             -> list[int]: output position o holds input perm[o], for cleartext signs per layer and switch
    mask_layer(ctx, inputs, bits, p, q, log2_stride, out=None)          -> (k, limbs): [b - p | (x - y) - q]; bits None: (k / 2, limbs)
    switch_layer(ctx, inputs, d, e, p, q, pq, log2_stride, out=None)    -> (k, limbs)
    async iterated_butterfly_network(co, inputs, bits, triples, open_bits="per_layer")   -> (k, limbs) shuffled shares
    async shuffle_and_open(co, inputs, bits, triples, open_bits="per_layer")             -> (shares, opened)

`bits`: (L, k / 2, limbs) this party's shares of the signs; `triples = (p, q, pq)`, each (L, k / 2, limbs); layer l uses row l
(one sign and one triple a switch).  Where preprocessing is stored is the caller's business.  The tensor-level functions run on
torch's current stream and nothing synchronises; every party runs the same coroutine over its OpenCoalescer, so the opens meet
batch for batch.

open_bits="per_layer" is the reference's traffic: one open of k elements a layer.  open_bits="upfront": b - p does not depend on
the data, so these differences are opened ahead of the layers that need them -- in slabs of whole layers under `slab_bytes`, the
first before layer 0 and each later one in the same batch as the last layer of the slab before it -- and every layer opens only
its k / 2 data-dependent elements.  Same result bit for bit, the same values revealed (only earlier), half the bytes and half the
decode work on the path of each round.
"""
from .share_arithmetic import _out, sub

SLAB_BYTES = 256 << 20      # "upfront": most bytes of sign differences opened in one batch (whole layers; at least one)
_MODES = ("per_layer", "upfront")


def _log2(k):
    if not isinstance(k, int) or k < 2 or k & (k - 1):
        raise ValueError(f"k must be a power of two >= 2, got {k!r}")
    return k.bit_length() - 1


def _stride(k, log2_stride):
    n = _log2(k)
    if not isinstance(log2_stride, int) or not 0 <= log2_stride < n:
        raise ValueError(f"log2_stride must be in [0, {n}) for k = {k}, got {log2_stride!r}")
    return log2_stride


def layers(k):
    """log2_stride of every layer, in the reference's order: log2(k) iterations of 0, 1, ..., log2(k) - 1"""
    n = _log2(k)
    return [a for _ in range(n) for a in range(n)]


def switch_indices(k, log2_stride):
    """(xi, yi): switch j of a layer with stride 2^log2_stride reads inputs xi[j] and yi[j] (and writes outputs 2j, 2j + 1)"""
    a = _stride(k, log2_stride)
    xi = [((j >> a) << (a + 1)) | (j & ((1 << a) - 1)) for j in range(k // 2)]
    return xi, [x | (1 << a) for x in xi]


def permutation(k, signs):
    """The permutation the network applies for cleartext signs: signs[l][j] in {1, -1} for layer l (order of layers(k)) and
    switch j.  -> perm with output[o] = input[perm[o]]."""
    order = layers(k)
    if len(signs) < len(order):
        raise ValueError(f"signs: {len(order)} layers needed, got {len(signs)}")
    cur = list(range(k))
    for a, row in zip(order, signs):
        if len(row) != k // 2 or any(b not in (1, -1) for b in row):
            raise ValueError(f"signs: every layer takes {k // 2} values 1 or -1")
        xi, yi = switch_indices(k, a)
        nxt = [0] * k
        for j, b in enumerate(row):
            first, second = (xi[j], yi[j]) if b == 1 else (yi[j], xi[j])
            nxt[2 * j], nxt[2 * j + 1] = cur[first], cur[second]
        cur = nxt
    return cur


def _inputs(ctx, inputs, log2_stride):
    inputs = ctx.elems(inputs, what="inputs")
    k = inputs.numel() // ctx.n_limbs
    return inputs, k, _stride(k, log2_stride)


def _apart(ctx, out, inputs, count):
    """out (count elements) must not share memory with the layer's inputs: a switch writes positions other switches read"""
    a, b = out.data_ptr(), inputs.data_ptr()
    if a < b + inputs.numel() * 8 and b < a + count * ctx.nbytes:
        raise ValueError("out: must not overlap inputs (a layer is not computed in place)")
    return out


def mask_layer(ctx, inputs, bits, p, q, log2_stride, out=None):
    """Before a layer's open: [bits - p | in[xi] - in[yi] - q] as ONE (k, limbs) array; bits None (the signs' differences were
    opened in advance): (k / 2, limbs), the data-dependent half alone (p is not read).  One fused launch."""
    inputs, k, a = _inputs(ctx, inputs, log2_stride)
    half = k // 2
    q = ctx.elems(q, half, what="q")
    if bits is not None:
        bits, p = ctx.elems(bits, half, what="bits"), ctx.elems(p, half, what="p")
    count = k if bits is not None else half
    out = ctx.empty(count) if out is None else _apart(ctx, _out(ctx, out, inputs, count), inputs, count)
    ctx.check(ctx.lib.hb_bf_mask(ctx.h, ctx.ptr(inputs), None if bits is None else ctx.ptr(bits), None if bits is None else ctx.ptr(p), ctx.ptr(q),
                                 k, a, ctx.ptr(out), ctx.stream()), "hb_bf_mask")
    return out


def switch_layer(ctx, inputs, d, e, p, q, pq, log2_stride, out=None):
    """After a layer's open: d, e the opened b - p and (x - y) - q, (p, q, pq) this party's shares of the layer's triples.
    -> (k, limbs): out[2j] = (x + y + m) / 2, out[2j + 1] = (x + y - m) / 2 with m = d e + d q + e p + pq.  One fused launch;
    out must not be inputs."""
    inputs, k, a = _inputs(ctx, inputs, log2_stride)
    half = k // 2
    d, e, p, q, pq = (ctx.elems(v, half, what=w) for v, w in ((d, "d"), (e, "e"), (p, "p"), (q, "q"), (pq, "pq")))
    out = ctx.empty(k) if out is None else _apart(ctx, _out(ctx, out, inputs, k), inputs, k)
    ctx.check(ctx.lib.hb_bf_switch(ctx.h, ctx.ptr(inputs), ctx.ptr(d), ctx.ptr(e), ctx.ptr(p), ctx.ptr(q), ctx.ptr(pq), k, a, ctx.ptr(out), ctx.stream()),
              "hb_bf_switch")
    return out


def _preprocessing(ctx, k, bits, triples):
    order = layers(k)
    half, t = k // 2, ctx.torch
    try:
        p, q, pq = triples
    except (TypeError, ValueError):
        raise ValueError("triples: expected (p, q, pq)") from None
    rows = []
    for v, w in ((bits, "bits"), (p, "triples p"), (q, "triples q"), (pq, "triples pq")):
        if not isinstance(v, t.Tensor) or v.dim() != 3 or v.shape[1] != half or v.shape[2] != ctx.n_limbs:
            raise ValueError(f"{w}: expected a tensor of shape (layers, {half}, {ctx.n_limbs})")
        if v.shape[0] < len(order):
            raise ValueError(f"{w}: k = {k} takes {len(order)} layers, got {v.shape[0]} rows")
        rows.append(ctx.elems(v, what=w))
    return order, rows


async def iterated_butterfly_network(co, inputs, bits, triples, open_bits="per_layer", slab_bytes=SLAB_BYTES):
    """Shares of the k inputs, shuffled by the network the signs select (iterated_butterfly_network of the reference, with its
    batch_switch): log2(k)^2 rounds of mask_layer, one coalesced open, switch_layer.  inputs is left untouched; the layers
    ping-pong between two buffers of their own."""
    ctx = co.ctx
    if open_bits not in _MODES:
        raise ValueError(f"open_bits: one of {_MODES}, got {open_bits!r}")
    inputs = ctx.elems(inputs, what="inputs")
    k = inputs.numel() // ctx.n_limbs
    order, (bits, p, q, pq) = _preprocessing(ctx, k, bits, triples)
    half, n_layers = k // 2, len(order)
    buffers = [ctx.empty(k), ctx.empty(k)]
    cur = inputs
    if open_bits == "per_layer":
        for l, a in enumerate(order):
            opened = await co.open_share_array(mask_layer(ctx, cur, bits[l], p[l], q[l], a))
            cur = switch_layer(ctx, cur, opened[:half], opened[half:], p[l], q[l], pq[l], a, out=buffers[l & 1])
        return cur
    per_slab = max(1, int(slab_bytes) // (half * ctx.nbytes))

    def open_slab(first):
        last = min(first + per_slab, n_layers)
        return first, co.open_share_array(sub(ctx, bits[first:last].reshape(-1, ctx.n_limbs), p[first:last].reshape(-1, ctx.n_limbs)))

    first, pending = open_slab(0)
    d_slab = (await pending).reshape(-1, half, ctx.n_limbs)
    for l, a in enumerate(order):
        e_open = co.open_share_array(mask_layer(ctx, cur, None, None, q[l], a))
        nxt = None
        if l + 1 == first + per_slab and l + 1 < n_layers:
            nxt = open_slab(l + 1)                  # queued before the await below: it travels with this layer's open
        e = await e_open
        cur = switch_layer(ctx, cur, d_slab[l - first], e, p[l], q[l], pq[l], a, out=buffers[l & 1])
        if nxt is not None:
            first, d_slab = nxt[0], (await nxt[1]).reshape(-1, half, ctx.n_limbs)
    return cur


async def shuffle_and_open(co, inputs, bits, triples, open_bits="per_layer", slab_bytes=SLAB_BYTES):
    """butterfly_network_helper of the reference: the shuffled shares and their opened values"""
    shares = await iterated_butterfly_network(co, inputs, bits, triples, open_bits=open_bits, slab_bytes=slab_bytes)
    return shares, await co.open_share_array(shares)
