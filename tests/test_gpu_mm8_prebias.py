"""Element buffers that are biased and interleaved once, where an element enters LDS (k_mm8<.., PB> behind its DMA, k_mm8f's MSC = 1 scaling
tasks), and the phases that read them as they lie (gen_mm8.py: Mm8PhaseB, Mm8PhasePackedB).  What can go wrong is a byte that is biased
twice or not at all, a dword of the wrong element or the wrong half in a granule, a K-block transformed by nobody or by two waves, and a
transform of one LDS buffer that meets the passes over the other -- so:

k_mm8 on its own (hb_debug_mm8_*), Vandermonde rows at 1 .. n over BLS12-381 r:
    d = 5, 9, 22, 32        one to four K-blocks (the skip of K-block 0's second digit group from two on)
    n = 16, 22, 40, 64      one to four row tiles, 22 and 40 with a ragged last tile; four, two, one tile a unit
                            All pairs that the library builds an image for: (16, 22) and (16, 32) pass the kernel's LDS budget (four
                            tiles a unit of three or four K-blocks), and x^31 at x = 22, 40, 64 passes the 2^126 an entry may have --
                            hb_debug_mm8_create refuses those five, and no caller ever runs them.  Four K-blocks at the points 1 .. n
                            are n = 33 .. 38 with d = 25 (38^24 < 2^126, three row tiles): (36, 25), a ragged last tile of four rows
    chunks 1, 15, 17, 65 and one count past two units a workgroup (the second unit lies in the other buffer), both output layouts
    inputs: every byte 0x00 / 0x7f / 0x80 / 0xff (any 256-bit value is a legal input), one distinct byte per position, 0, 1, p - 1, random
  Every output is compared with sum(x_i^l a_l) mod p in Python integers: 65 distinct chunks are computed once, a launch's chunk k holds
  chunk k mod 65 (65 is prime to every unit size), and all of its outputs are compared.  HB_MM8_NO_PREBIAS=1 (the image is then built for
  the raw layout) gives the same bytes.

k_mm8f with MSC = 1 through BatchOpen plans: (n, t) = (13, 4), (16, 5), (31, 10), (64, 21) at the points i + 1 -- d = 5, 6, 11, 22: one
to three K-blocks and all three forms of the last row tile -- C = 1, 63, 65 and two units a workgroup, seeded arrival orders, messages at
the edges of the arithmetic (edge_values, structured).  The results equal the secrets and the R2 message the constant terms bit for bit,
ok() holds, one changed element of a compared or of a decoded column clears it, and HB_NO_FUSED_MSCALE=1 (the raw layout) gives the same."""
import ctypes
import random

import numpy as np
import pytest

import edge_values
import structured
from conftest import BLS, clear_hook, set_hook

pytestmark = pytest.mark.gpu

P = BLS
BASE = 65
MM8_D = [5, 9, 22, 32]
MM8_N = [16, 22, 40, 64]
MM8_TOO_LARGE = {(16, 22), (16, 32), (22, 32), (40, 32), (64, 32)}
MM8_CASES = [(n, d) for n in MM8_N for d in MM8_D if (n, d) not in MM8_TOO_LARGE] + [(36, 25)]
MM8_CHUNKS = [1, 15, 17, 65]
FS_SHAPES = [(13, 4), (16, 5), (31, 10), (64, 21)]
FS_CHUNKS = [1, 63, 65, None]          # None: one count past a second unit for some workgroup
_mm8_inputs = {}
_fs_inputs = {}


def _cus():
    import torch

    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _limbs(values):
    """256-bit values as they are, no reduction: (len, 4) uint64"""
    arr = np.zeros((len(values), 4), dtype=np.uint64)
    for k, v in enumerate(values):
        for j in range(4):
            arr[k, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return arr


def _mm8_base(d):
    """BASE chunks of d elements: the byte patterns first (alone in a chunk, then mixed), then residues"""
    if d not in _mm8_inputs:
        rnd = random.Random(4100 + d)
        distinct = sum((a + 1) << (8 * a) for a in range(32))
        pats = [0, int("7f" * 32, 16), int("80" * 32, 16), int("ff" * 32, 16), distinct, 1, P - 1]
        chunks = [[v] * d for v in pats]
        chunks += [[pats[(k + l) % len(pats)] for l in range(d)] for k in range(len(pats))]
        chunks += [[rnd.choice(pats) if rnd.random() < 0.5 else rnd.randrange(P) for _ in range(d)] for _ in range(16)]
        chunks += [[rnd.randrange(1 << 256) for _ in range(d)] for _ in range(8)]
        chunks += [[rnd.randrange(P) for _ in range(d)] for _ in range(BASE - len(chunks))]
        assert len(chunks) == BASE
        _mm8_inputs[d] = chunks
    return _mm8_inputs[d]


def test_k_mm8_shapes_left_out_are_refused_by_the_library():
    from honeybadgermpc_amd._capi import Context, np_ptr

    ctx = Context.get(P)
    for n, d in sorted(MM8_TOO_LARGE):
        h = ctypes.c_void_p()
        assert ctx.lib.hb_debug_mm8_create(ctx.h, np_ptr(ctx.host_elems(list(range(1, n + 1)))), n, d, ctypes.byref(h)) == 3      # HB_ERR_UNSUPPORTED


@pytest.mark.parametrize("n,d", MM8_CASES)
def test_k_mm8_prebiased_against_python_ints(monkeypatch, n, d):
    import torch

    from honeybadgermpc_amd._capi import Context, np_ptr

    ctx = Context.get(P)
    lib = ctx.lib
    base = _mm8_base(d)
    pts = list(range(1, n + 1))
    pw = [[pow(x, l, P) for l in range(d)] for x in pts]
    want = [[sum(pw[i][l] * ch[l] for l in range(d)) % P for i in range(n)] for ch in base]         # [chunk][row]: all of them
    want_dev = ctx.to_device(_limbs([v for row in want for v in row])).view(BASE, n, 4)
    in_dev = ctx.to_device(_limbs([v for ch in base for v in ch])).view(BASE, d, 4)
    n_rt = (n + 15) // 16
    tpw = {1: 4, 2: 2}.get(n_rt, 1)
    two_units = 16 * tpw * (2 * _cus()) + 1          # one chunk past a full round of units: some workgroup takes a second unit
    results = {}
    for prebias in (True, False):
        if prebias:
            clear_hook(monkeypatch, "HB_MM8_NO_PREBIAS")
        else:
            set_hook(monkeypatch, "HB_MM8_NO_PREBIAS", "1")
        h = ctypes.c_void_p()
        ctx.check(lib.hb_debug_mm8_create(ctx.h, np_ptr(ctx.host_elems(pts)), n, d, ctypes.byref(h)), "mm8 table")     # (the hook is read here)
        for chunks in MM8_CHUNKS + [two_units]:
            reps = (chunks + BASE - 1) // BASE
            x_dev = in_dev.repeat(reps, 1, 1)[:chunks].contiguous()
            exp = want_dev.repeat(reps, 1, 1)[:chunks].contiguous()
            for party_major in (True, False):
                out = ctx.empty(chunks * n)
                out.fill_(-1)
                sc, sl = (1, chunks) if party_major else (n, 1)
                ctx.check(lib.hb_debug_mm8_apply(ctx.h, h, ctx.ptr(x_dev), d, 1, chunks * d, ctx.ptr(out), sc, sl, chunks * n, chunks, None, None), "mm8 apply")
                torch.cuda.synchronize()
                got = out.view(n, chunks, 4).transpose(0, 1) if party_major else out.view(chunks, n, 4)
                if not torch.equal(got, exp):
                    bad = (got != exp).any(dim=2).nonzero()[0].tolist()
                    raise AssertionError(f"prebias={prebias} chunks={chunks} party_major={party_major}: first wrong (chunk, row) = {bad}")
                results[(prebias, chunks, party_major)] = out
    for (prebias, chunks, party_major), out in results.items():
        if prebias:
            assert torch.equal(out, results[(False, chunks, party_major)])


def _fs_base(n, t):
    """BASE messages of d coefficients and their codewords: values at chosen points on the edges, coefficients on the edges, the
    structured kinds; -> (rows [BASE][d], codewords [BASE][n])"""
    if (n, t) not in _fs_inputs:
        d = t + 1
        x = list(range(1, n + 1))
        rnd = random.Random(97 * n + t)
        where = rnd.sample(range(n), d)
        rows = edge_values.targeted_rows(P, x, where, d, 36, seed=n)
        rows += edge_values.edge_rows(P, d, 17, seed=t)
        rows += structured.structured_rows(rnd, P, BASE - len(rows), d)
        assert len(rows) == BASE
        _fs_inputs[(n, t)] = (rows, edge_values.evaluate_rows(P, x, rows))
    return _fs_inputs[(n, t)]


@pytest.mark.parametrize("ci", range(len(FS_CHUNKS)))
@pytest.mark.parametrize("n,t", FS_SHAPES)
def test_k_mm8f_prebiased_through_open_plans(monkeypatch, n, t, ci):
    import torch

    from honeybadgermpc_amd._capi import Context, load_library
    from honeybadgermpc_amd.device import BatchOpen

    ctx = Context.get(P)
    d = t + 1
    c = FS_CHUNKS[ci] if FS_CHUNKS[ci] is not None else 64 * _cus() + 1
    b = c * d
    rows, enc = _fs_base(n, t)
    order = list(range(n))
    random.Random(1000 * n + 10 * t + ci).shuffle(order)
    z, zc = order[:d], order[d : d + t]
    reps = (c + BASE - 1) // BASE
    cols = ctx.upload_ints([enc[k][j] for j in range(n) for k in range(BASE)]).view(n, BASE, 4).repeat(1, reps, 1)[:, :c].contiguous()
    want = ctx.upload_ints([v for row in rows for v in row]).view(BASE, d, 4).repeat(reps, 1, 1)[:c].contiguous()
    flat = cols.view(n * c, 4)
    seen = {}
    for on in (True, False):
        if on:
            clear_hook(monkeypatch, "HB_NO_FUSED_MSCALE")
        else:
            set_hook(monkeypatch, "HB_NO_FUSED_MSCALE", "1")
        op = BatchOpen(P, n, t, z=z, zc=zc, max_shares=b)           # (the hook is read when the plan builds its images)
        assert op.fused_validate_kernel() == "small"
        res = op.r2_decode(flat, b)
        assert load_library().hb_debug_fs_last_mscale() == (1 if on else 0)
        msg = op.r1_decode(flat, b)
        assert load_library().hb_debug_fs_last_mscale() == (1 if on else 0)
        assert op.ok()
        assert torch.equal(res.view(c, d, 4), want), (on, "secrets")
        assert torch.equal(msg.view(c, 4), want[:, 0, :]), (on, "R2 message")
        seen[on] = (res.clone(), msg.clone())
        # one element of one compared column, then one of one decoded column: either clears ok(), in both launches
        for sender, chunk in ((zc[ci % t], c - 1), (z[(ci + 1) % d], c // 2)):
            word = cols[sender, chunk, 1].clone()
            cols[sender, chunk, 1] ^= 1 << 7
            op.r2_decode(flat, b)
            assert not op.ok(), (on, sender, chunk, "r2")
            op.r1_decode(flat, b)
            assert not op.ok(), (on, sender, chunk, "r1")
            cols[sender, chunk, 1] = word
        op.r2_decode(flat, b)
        assert op.ok()
    assert torch.equal(seen[True][0], seen[False][0]) and torch.equal(seen[True][1], seen[False][1])
