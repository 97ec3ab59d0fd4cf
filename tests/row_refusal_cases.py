"""What the row steps refuse: one entry per step that has a step function (csrc/hb_rows.hpp), shared by test_row_refusals_host.py,
which drives the host self tests, and test_gpu_row_refusals.py, which drives the device entry points over the same table.

An entry names the step's operands in the order of its self test, each with its rows of `count` elements, and a legal argument set
at count = 3 with the smallest shape parameters the step takes.  mutations() lists single changes of that set with the code each
must give: an output laid over the first and over the last row of every input and of every other output, every shape parameter
one past each bound, every required operand null (refused) and every optional one null (accepted).  All operands of a call are
carved out of ONE buffer, so an output that is laid over an input really is."""
import ctypes
import random

import numpy as np

COUNT = 3
WIDE = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001      # the BLS12-381 scalar field, 4 limbs
NARROW = 0xFFFFFFFFFFFFFFC5                                                      # 1 limb
FIELDS = [(WIDE, 4), (NARROW, 1)]
OK, BAD_ARG = 0, 2


class Op:
    """name[:rows][flag] -- rows: an expression over the step's parameters, or i8 (one byte an element) / z (four bytes a row of
    `rows`); flag ? optional (null is accepted), ~ not looked at with these parameters (null is accepted, nothing may not lie over
    it), @ one element in host memory"""

    def __init__(self, text):
        self.flag = text[-1] if text[-1] in "?~@" else ""
        text = text.rstrip("?~@")
        self.name, _, self.rows = text.partition(":")
        self.rows = self.rows or "1"

    def nbytes(self, prm, eb):
        if self.rows == "i8":
            return COUNT
        if self.rows == "z":
            return 4 * prm["rows"]
        return (1 if self.flag == "@" else eval(self.rows, {}, dict(prm)) * COUNT) * eb


class Step:
    def __init__(self, entry, family, what, sparams, ins, outs, dev, params=None, bad=None, apart=True, alias=()):
        self.entry, self.family, self.what = entry, family, what
        self.sparams = sparams.split()                  # the self test's params[], names of parameters or numbers
        self.ins, self.outs = [Op(t) for t in ins.split()], [Op(t) for t in outs.split()]
        self.dev = dev.split()                          # the entry point's arguments after ctx and before stream
        self.params = params or {}                      # a value may be a function of bits(p)
        self.bad = bad or {}                            # parameter -> values one past its bounds
        self.apart = apart                              # False: the step lets outputs lie over inputs
        self.alias = alias                              # (output, operand): the same address is refused
        self.id = entry + "".join("-%s%s" % (k, v) for k, v in self.params.items() if not callable(v) and k in ("nodes", "root"))

    def values(self, p):
        return {k: v(p.bit_length()) if callable(v) else v for k, v in self.params.items()}

    def ops(self):
        return self.ins + self.outs


def _bits(d):
    return lambda bits: bits + d


S = Step
STEPS = [
    # ---- hb_lt.hip: params = L, mode
    S("hb_lt_mask", "lt", 0, "L 0", "a b? r", "masked", "a b r masked count", {"L": _bits(0)}),
    S("hb_lt_leaves", "lt", 1, "L mode", "c r_bits:L", "g:L p:L", "c r_bits L mode g p count", {"L": _bits(0), "mode": 0},
      {"L": [_bits(-1), _bits(1)], "mode": [-1, 2]}),
    S("hb_lt_xor_mask", "lt", 2, "L 0", "c r0 w pa qa", "u masked:2", "c r0 w pa qa u masked count", {"L": _bits(0)}),
    S("hb_lt_dmask", "lt", 3, "L 1", "c r0 x s s_bits:L pa qa pb qb", "u masked:5", "c r0 x s s_bits L pa qa pb qb u masked count", {"L": _bits(0)},
      {"L": [_bits(-1), _bits(1)]}),
    S("hb_lt_mid", "lt", 4, "L 1", "opened:5 u s_bits:L pa qa pqa pb qb pqb pc qc", "v d0 masked:2",
      "opened u s_bits L pa qa pqa pb qb pqb pc qc v d0 masked count", {"L": _bits(0)}, {"L": [_bits(-1), _bits(1)]}),
    S("hb_lt_xor_finish", "lt", 5, "L 0", "opened:2 u v p q pq", "out", "opened u v p q pq out count", {"L": _bits(0)}),
    # ---- hb_eq.hip: params = rows, mode
    S("hb_legendre", "eq", 0, "1 0", "a", "out:i8", "a out count"),
    S("hb_eq_mask1", "eq", 1, "rows 0", "x y? r:rows rp:rows pa:rows qa:rows pb:rows qb:rows", "masked:4*rows", "x y r rp pa qa pb qb masked rows count",
      {"rows": 2}, {"rows": [0, 4097]}),
    S("hb_eq_mid", "eq", 2, "rows 0", "opened:4*rows pa:rows qa:rows pqa:rows pb:rows qb:rows pqb:rows bits:rows pc:rows qc:rows nr@", "masked2:2*rows dr:rows",
      "opened pa qa pqa pb qb pqb bits pc qc nr masked2 dr rows count", {"rows": 2}, {"rows": [0, 4097]}),
    S("hb_eq_cshare", "eq", 3, "rows 0", "opened2:2*rows dr:rows pc:rows qc:rows pqc:rows", "c:rows", "opened2 dr pc qc pqc c rows count", {"rows": 2},
      {"rows": [0, 4097]}),
    S("hb_eq_finish", "eq", 4, "rows mode", "c:rows bits:rows nr@", "factor:rows zero_rows:z", "c bits mode nr factor zero_rows rows count", {"rows": 2, "mode": 1},
      {"rows": [0, 4097], "mode": [-1, 2]}),
    # ---- hb_fxp.hip: params = k, m, kappa, aux, root
    S("hb_fxp_mask", "fxp", 0, "k m kappa 0 0", "x? bits:k+kappa", "masked r1", "x bits k m kappa masked r1 count", {"k": 2, "m": 1, "kappa": 0},
      {"m": [0, 2], "kappa": [-1], "k": [_bits(-1)]}, apart=False, alias=[("masked", "r1")]),
    S("hb_fxp_trunc_pr", "fxp", 1, "0 m 0 0 0", "x c r1 inv2m@", "out", "x c r1 m inv2m out count", {"m": 1}, {"m": [0, _bits(-1)]}, apart=False),
    S("hb_fxp_ltl_leaves", "fxp", 2, "0 m 0 0 0", "c bits:m", "g:m+1 p:m+1", "c bits m g p count", {"m": 1}, {"m": [0, _bits(-1)]}),
    S("hb_fxp_carry_mask", "fxp", 3, "0 0 0 nodes root", "g:2 p:2 ta tb", "masked:2", "g p nodes root ta tb masked count", {"nodes": 2, "root": 1},
      {"nodes": [1, 3]}),
    S("hb_fxp_carry_mask", "fxp", 3, "0 0 0 nodes root", "g:3 p:3 ta:2 tb:2", "masked:4", "g p nodes root ta tb masked count", {"nodes": 3, "root": 0},
      {"nodes": [1, 258]}),
    S("hb_fxp_carry_combine", "fxp", 4, "0 0 0 nodes root", "opened:2 g:2 p:2 ta tb tab", "g_out p_out~", "opened g p nodes root ta tb tab g_out p_out count",
      {"nodes": 2, "root": 1}, {"nodes": [1, 3]}),
    S("hb_fxp_carry_combine", "fxp", 4, "0 0 0 nodes root", "opened:4 g:3 p:3 ta:2 tb:2 tab:2", "g_out:2 p_out:2", "opened g p nodes root ta tb tab g_out p_out count",
      {"nodes": 3, "root": 0}, {"nodes": [1, 258]}),
    S("hb_fxp_div2m_finish", "fxp", 5, "0 m 0 mode 0", "x c r1 carry inv2m@", "out", "x c r1 carry m inv2m mode out count", {"m": 1, "mode": 1},
      {"m": [0, _bits(-1)], "mode": [-1, 3]}, apart=False),
    # ---- hb_bd.hip: params = m, level
    S("hb_bd_leaves", "bd", 0, "m 0", "c bits:m-1", "g:m-1 p:m-1", "c bits m g p count", {"m": 2}, {"m": [0, _bits(-1)]}),
    S("hb_bd_prefix_mask", "bd", 1, "m level", "g:2 p:2 ta tb", "masked:2", "g p m level ta tb masked count", {"m": 3, "level": 0},
      {"m": [0, _bits(-1)], "level": [-1, 1]}),
    S("hb_bd_prefix_combine", "bd", 2, "m level", "opened:2 ta tb tab", "g:2 p:2", "opened g p m level ta tb tab count", {"m": 3, "level": 0},
      {"m": [0, _bits(-1)], "level": [-1, 1]}),
    S("hb_bd_sum_mask", "bd", 3, "m 0", "c bits:m g:m-1 ta:m-1 tb:m-1", "masked:2*(m-1)", "c bits g m ta tb masked count", {"m": 2}, {"m": [0, _bits(-1)]}),
    S("hb_bd_sum_combine", "bd", 4, "m 0", "opened:2*(m-1) c bits:m g:m-1 ta:m-1 tb:m-1 tab:m-1", "out:m", "opened c bits g m ta tb tab out count", {"m": 2},
      {"m": [0, _bits(-1)]}),
    # ---- hb_div.hip: params as the header lists them for each step
    S("hb_div_or_mask", "div", 0, "n_planes level 0", "y:2 ta tb", "masked:2", "y n_planes level 0 ta tb masked count", {"n_planes": 2, "level": 0},
      {"n_planes": [0, 257], "level": [-1, 1]}),
    S("hb_div_or_combine", "div", 1, "n_planes level 0", "opened:2 ta tb tab", "y:2", "opened y n_planes level 0 ta tb tab count", {"n_planes": 2, "level": 0},
      {"n_planes": [0, 257], "level": [-1, 1]}),
    S("hb_div_pair_mask", "div", 5, "0", "x y ta tb", "masked:2", "x y ta tb masked count"),
    S("hb_div_norm_mask", "div", 2, "n_planes", "x y u? ta:2 tb:2", "masked:4 v", "x y n_planes u ta tb masked v count", {"n_planes": 1}, {"n_planes": [0, 257]}),
    S("hb_div_product_step", "div", 3, "mode products 0 0 0", "opened:2 ta tb tab aux cst~ nxt_a~ nxt_b~ bits~", "out0 out1~",
      "mode products opened ta tb tab aux cst nxt_a nxt_b bits 0 0 0 out0 out1 count", {"mode": 0, "products": 1}, {"mode": [-1, 4], "products": [0, 2]}),
    S("hb_div_trunc_step", "div", 4, "mode rows products m", "opened s inv2m@ alpha~ x~ ext0~ ext1~ ta~ tb~", "out",
      "mode rows products opened s m inv2m alpha x ext0 ext1 ta tb out count", {"mode": 0, "rows": 1, "products": 0, "m": 1},
      {"mode": [-1, 3], "rows": [0, 2], "products": [1], "m": [0, _bits(-1)]}),
    # ---- hb_sort.hip: params = n, batch, width, a, r, d, cnt, k, kappa; count = batch cnt, and n rows of `batch` are a column
    S("hb_sort_cmp_mask", "sort", 0, "n 3 1 0 0 d 1 k kappa", "table:n bits:k+kappa", "masked r1", "table n 3 0 0 d 1 bits k kappa masked r1",
      {"n": 2, "d": 1, "k": 2, "kappa": 0}, {"n": [1], "d": [0, 2], "k": [1, _bits(-1)], "kappa": [-1]}),
    S("hb_sort_swap_mask", "sort", 1, "n 3 width 0 0 d 1 k 0", "table:n*width c r1 carry p:width q:width inv2m@", "out:2*width",
      "table width n 3 0 0 d 1 c r1 carry p q k inv2m out", {"n": 2, "d": 1, "width": 1, "k": 2}, {"n": [1], "d": [0, 2], "width": [0, 257], "k": [1, _bits(0)]}),
    S("hb_sort_swap_finish", "sort", 2, "n 3 width 0 0 d 1 0 0", "opened:2*width p:width q:width pq:width", "table:n*width", "table width n 3 0 0 d 1 opened p q pq",
      {"n": 2, "d": 1, "width": 1}, {"n": [1], "d": [0, 2], "width": [0, 257]}),
    # ---- hb_demux.hip: params = m, level
    S("hb_demux_leaves", "demux", 0, "0 0", "bits", "out:2", "bits out count"),
    S("hb_demux_mask", "demux", 1, "m level", "bits:m groups~ ta:4", "out:4", "bits groups m level ta out count", {"m": 2, "level": 0},
      {"m": [0, 13], "level": [-1, 1]}),
    S("hb_demux_finish", "demux", 2, "m level", "opened:4 ta:4 tab:4", "groups:4", "opened ta tab m level groups count", {"m": 2, "level": 0},
      {"m": [0, 13], "level": [-1, 1]}),
]
HAS_COUNT = {"sort": False}                         # hb_selftest_sort and the sort entry points take no count


def mutations(step, p):
    """-> [(label, change, code)]; change: ("over", output, operand, "first" | "last"), ("same", output, operand), ("null", operand)
    or ("param", name, value)"""
    out = []
    for o in step.outs:
        if o.flag == "~":
            continue
        targets = [t for t in step.ops() if t is not o and t.flag not in ("~", "@")] if step.apart else []
        out += [("%s over the %s row of %s" % (o.name, where, t.name), ("over", o.name, t.name, where), BAD_ARG) for t in targets for where in ("first", "last")]
    out += [("%s is %s" % pair, ("same",) + tuple(pair), BAD_ARG) for pair in step.alias]
    out += [("%s null" % t.name, ("null", t.name), OK if t.flag in ("?", "~") else BAD_ARG) for t in step.ops()]
    for name, values in step.bad.items():
        for v in values:
            v = v(p.bit_length()) if callable(v) else v
            out.append(("%s = %d" % (name, v), ("param", name, v), BAD_ARG))
    return out


class Call:
    """One argument set of a step: where every operand lies in the one buffer (an offset, or None for a null operand), the step's
    parameters, and the contents of the buffer before the call."""

    def __init__(self, step, p, nl, change=None, seed=1):
        self.step, self.p, self.nl, self.eb = step, p, nl, 8 * nl
        self.prm = step.values(p)
        sizes = {t.name: t.nbytes(self.prm, self.eb) for t in step.ops()}
        slack = max(sizes[o.name] for o in step.outs) + 64
        self.off, at = {}, slack
        for t in step.ops():
            self.off[t.name] = at
            at += (sizes[t.name] + 63) // 64 * 64
        self.sizes, self.total = sizes, at + slack
        if change and change[0] == "over":
            _, o, t, where = change
            self.off[o] = self.off[t] + sizes[t] - self.eb if where == "last" else self.off[t] - max(sizes[o] - self.eb, 0)
        elif change and change[0] == "same":
            self.off[change[1]] = self.off[change[2]]
        elif change and change[0] == "null":
            self.off[change[1]] = None
        elif change and change[0] == "param":
            self.prm[change[1]] = change[2]
        # inputs: residues below p; outputs: the sentinel (legal=True fills them as the existing drivers do)
        rnd = random.Random(seed)
        self.inputs = {t.name: [rnd.randrange(p) for _ in range(sizes[t.name] // self.eb)] for t in step.ins}
        self.initial = {o.name: [rnd.randrange(p) for _ in range(sizes[o.name] // self.eb)] for o in step.outs if o.rows not in ("i8", "z")}

    def buffer(self, sentinel=True):
        """the buffer before the call: inputs first, then the outputs' fill wherever they lie (a refused call leaves all of it)"""
        from honeybadgermpc_amd._capi import ints_to_limbs

        buf = np.full(self.total, 0xA5, dtype=np.uint8)
        for t in self.step.ins:
            if self.off[t.name] is not None:
                raw = ints_to_limbs(self.inputs[t.name], self.p, self.eb).tobytes()
                buf[self.off[t.name]:self.off[t.name] + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        for o in self.step.outs:
            if self.off[o.name] is None:
                continue
            lo, n = self.off[o.name], self.sizes[o.name]
            if sentinel:
                buf[lo:lo + n] = 0x5A
            elif o.rows == "i8":
                buf[lo:lo + n] = 7
            elif o.rows == "z":
                buf[lo:lo + n] = 0
            else:
                buf[lo:lo + n] = np.frombuffer(ints_to_limbs(self.initial[o.name], self.p, self.eb).tobytes(), dtype=np.uint8)
        return buf

    def address(self, name, base, host_base=None):
        """the operand's address for a buffer at `base`; an @ operand stays in host memory (host_base)"""
        if self.off[name] is None:
            return None
        op = next(t for t in self.step.ops() if t.name == name)
        return (host_base if op.flag == "@" and host_base is not None else base) + self.off[name]

    def output(self, buf, name):
        return buf[self.off[name]:self.off[name] + self.sizes[name]]

    def selftest(self, buf):
        """the host self test over `buf` (changed in place) -> rc"""
        from honeybadgermpc_amd._capi import ints_to_limbs, load_library, np_ptr

        lib, base, step = load_library(), buf.ctypes.data, self.step
        ops = (ctypes.c_void_p * 12)(*[self.address(t.name, base) for t in step.ins])
        outs = (ctypes.c_void_p * 3)(*[self.address(o.name, base) for o in step.outs])
        prm = (ctypes.c_int64 * 9)(*[self.prm[s] if s in self.prm else int(s) for s in step.sparams])
        args = [np_ptr(ints_to_limbs([self.p], self.p + 1, self.eb)), self.nl, step.what, ops, prm, outs]
        return getattr(lib, "hb_selftest_" + step.family)(*args + ([COUNT] if HAS_COUNT.get(step.family, True) else []))

    def device(self, ctx, base, host_base):
        """the device entry point over a device buffer at `base` (host_base: the host copy, for the @ operands) -> rc"""
        names = {t.name for t in self.step.ops()}
        args = []
        for a in self.step.dev:
            if a in names:
                args.append(self.address(a, base, host_base))
            else:
                args.append(COUNT if a == "count" else self.prm[a] if a in self.prm else int(a))
        return getattr(ctx.lib, self.step.entry)(ctx.h, *args, None)


def driver_outputs(call):
    """the legal set through the existing driver of the step's family -> {output: bytes}"""
    import bitdec_cases
    import demux_cases
    import division_cases
    import selftest_cases
    import sort_cases
    from honeybadgermpc_amd._capi import ints_to_limbs

    step, p, nl, prm = call.step, call.p, call.nl, call.prm
    operands = [call.inputs[t.name] for t in step.ins]
    sparams = [prm[s] if s in prm else int(s) for s in step.sparams]
    rows = [o.rows if o.rows in ("i8", "z") else call.sizes[o.name] // call.eb // COUNT for o in step.outs]
    if step.family == "lt":
        rc, res = selftest_cases.run_lt(p, nl, step.what, operands, sparams[1], rows, COUNT, L=sparams[0])
    elif step.family == "eq":
        rc, res = selftest_cases.run_eq(p, nl, step.what, operands, sparams[0], sparams[1], ["zr" if r == "z" else r for r in rows], COUNT)
    elif step.family == "sort":
        rc, res = sort_cases.run_sort(p, nl, step.what, operands, sparams[0], sparams[1], sparams[2], tuple(sparams[3:7]), sparams[7], sparams[8],
                                      [call.initial[o.name] for o in step.outs])
    else:
        run = {"fxp": bitdec_cases.run_fxp, "bd": bitdec_cases.run_bd, "div": division_cases.run_div, "demux": demux_cases.run_demux}[step.family]
        rc, res = run(p, nl, step.what, operands, sparams, [call.initial[o.name] for o in step.outs], COUNT)
    assert rc == OK, (step.id, rc)
    out = {}
    for o, r, values in zip(step.outs, rows, res):
        if r == "i8":
            out[o.name] = np.array(values, dtype=np.int8).tobytes()
        elif r == "z":
            out[o.name] = np.array(values, dtype=np.int32).tobytes()
        else:
            out[o.name] = ints_to_limbs(values, p, call.eb).tobytes()
    return out
