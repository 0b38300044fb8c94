"""Shared by tests/test_air_program_fuzz.py and tests/test_gpu_air_program_fuzz.py:
a seeded generator of raw LSP_AIR_PROGRAM configs -- op tuples written directly,
not through ProgramBuilder, so they hold what the format of include/lsp.h allows
and the builder never emits (dst equal to an operand slot, both operands the
same, CONST op CONST, selector op selector, an ASSERT_ZERO straight on any
operand kind, a slot overwritten and read again) -- with the fixed corpus made
from it, edge-laden values for cells, constants and public values, and the
big-integer references of the check report and of the pointwise quotient.

Three families (free, identity, solvable: see the functions).  Every value is
canonical (< r): non-canonical cells are out of scope here.  Nothing here calls
the library; only air.py and field.py are imported from the package."""
import copy
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import preprocessed_ref as PR  # noqa: E402
from linea_stark_prover_amd.air import AirProgramConfig, LineaAIR, lower, permutation_air  # noqa: E402
from linea_stark_prover_amd.field import GENERATOR, MODULUS, to_mont, two_adic_generator  # noqa: E402

R = MODULUS
PD = 1           # public_degree of the default StarkConfig
MAX_DEG = 9      # 2^log_blowup + 1
NPUB = 4         # [alpha, delta] and two extra public values
ADD, SUB, MUL, ASSERT = 1, 2, 3, 4
SLOT, LOCAL, NEXT, PUBLIC, CONST, FIRST, LAST, TRANS, PREP_LOCAL, PREP_NEXT = range(10)
LEAF_DEG = {LOCAL: 1, NEXT: 1, PUBLIC: PD, CONST: 0, FIRST: 1, LAST: 1, TRANS: 0, PREP_LOCAL: 1, PREP_NEXT: 1}

_R256 = pow(2, 256, R)
EDGES = [0, 1, 2, R - 1, R - 2, (R + 1) // 2, (R - 1) // 2, 1 << 252, _R256, pow(2, 261, R), R - _R256,
         pow(pow(2, 261, R), R - 2, R)]


def draw_value(rng):
    """a canonical value: about 0.4 from the edge pool, else uniform below r"""
    return rng.choice(EDGES) if rng.random() < 0.4 else rng.randrange(R)


def draw_rows(rng, h, w):
    return [[draw_value(rng) for _ in range(w)] for _ in range(h)]


def kind(x):
    return x >> 24


def regime(nslots):
    return "nslots_0" if nslots == 0 else "nslots_1_5" if nslots <= 5 else "nslots_6_8" if nslots <= 8 else \
        "nslots_9_16"


# ---------------------------------------------------------------- generator
class _Gen:
    """op list under construction: which slots are written and every slot's
    degree under the rule of preprocessed_ref.program_degrees"""

    def __init__(self, rng, width, nslots, prep_width=0, cols=None, kinds=None):
        self.rng, self.width, self.nslots, self.wp = rng, width, nslots, prep_width
        self.cols = list(range(width)) if cols is None else cols
        self.kinds = kinds or [LOCAL, NEXT, PUBLIC, CONST, FIRST, LAST, TRANS] + ([PREP_LOCAL, PREP_NEXT] * 2
                                                                                    if prep_width else [])
        self.consts, self.ops, self.deg = [], [], [None] * nslots
        self.assert_deg = []
        self.draws = self.redraws = 0

    def const(self, v):
        if v not in self.consts:
            self.consts.append(v)
        return CONST << 24 | self.consts.index(v)

    def leaf(self, k=None):
        rng = self.rng
        k = rng.choice(self.kinds) if k is None else k
        if k in (LOCAL, NEXT):
            return k << 24 | rng.choice(self.cols)
        if k == PUBLIC:
            return k << 24 | rng.randrange(NPUB)
        if k == CONST:
            return self.const(draw_value(rng))
        if k in (PREP_LOCAL, PREP_NEXT):
            return k << 24 | rng.randrange(self.wp)
        return k << 24

    def written(self):
        return [s for s in range(self.nslots) if self.deg[s] is not None]

    def operand(self, p_slot=0.55):
        w = self.written()
        return self.rng.choice(w) if w and self.rng.random() < p_slot else self.leaf()

    def degree(self, x):
        return self.deg[x & 0xFFFFFF] if kind(x) == SLOT else LEAF_DEG[kind(x)]

    def op(self, code, dst, a, b, maxdeg=MAX_DEG):
        """append the op unless its degree passes maxdeg (a draw to redraw)"""
        self.draws += 1
        d = self.degree(a) + self.degree(b) if code == MUL else max(self.degree(a), self.degree(b))
        if d > maxdeg:
            self.redraws += 1
            return False
        self.ops.append((code, dst, a, b))
        self.deg[dst] = d
        return True

    def must(self, code, dst, a, b):
        ok = self.op(code, dst, a, b)
        assert ok, "a gadget passed the degree bound"

    def assert_zero(self, a):
        self.assert_deg.append(self.degree(a))
        self.ops.append((ASSERT, 0, a, 0))

    def random_op(self, maxdeg=MAX_DEG):
        rng = self.rng
        for _ in range(200):
            code, dst = rng.choice([ADD, SUB, MUL, MUL]), rng.randrange(self.nslots)
            a, b, form = self.operand(), self.operand(), rng.random()
            if form < 0.12:
                b = a                                           # both operands the same
            elif form < 0.19:
                a, b = self.leaf(CONST), self.leaf(CONST)       # CONST op CONST
            elif form < 0.26 and FIRST in self.kinds:
                a, b = rng.choice([FIRST, LAST, TRANS]) << 24, rng.choice([FIRST, LAST, TRANS]) << 24
            elif form < 0.42 and self.deg[dst] is not None:
                a = dst                                         # dst is an operand slot
                if rng.random() < 0.3:
                    b = dst
            elif form < 0.5 and self.deg[dst] is not None and code == SUB:
                b = dst
            if self.op(code, dst, a, b, maxdeg):
                return
        self.must(ADD, rng.randrange(self.nslots), self.leaf(CONST), self.leaf(CONST))

    def chain(self):
        """>= 8 ADD / SUB over products: s = l l, then s = s +- (l l) or s +- l"""
        rng = self.rng
        s = rng.randrange(self.nslots)
        self.must(MUL, s, self.leaf(), self.leaf())
        others = [x for x in range(self.nslots) if x != s]
        for _ in range(rng.randint(8, 12)):
            if others and rng.random() < 0.7:
                t = rng.choice(others)
                self.must(MUL, t, self.leaf(), self.leaf())
                self.must(rng.choice([ADD, SUB]), s, s, t)      # the subtrahend is a raw product
            else:
                self.must(rng.choice([ADD, SUB]), s, s, self.leaf())
        return s

    def pow9(self):
        """raw products multiplied up to degree 9 in two slots"""
        s, t = self.rng.sample(range(self.nslots), 2)
        self.must(MUL, s, self.leaf(), self.leaf())
        self.must(MUL, t, self.leaf(), self.leaf())
        self.must(MUL, s, s, t)             # <= 4
        self.must(MUL, t, s, self.leaf())   # <= 5
        self.must(MUL, s, s, t)             # <= 9: two raw products
        return s

    def build(self, family):
        cfg = AirProgramConfig(self.width, self.nslots, list(self.consts), list(self.ops), prep_width=self.wp)
        cfg.fuzz = dict(family=family, degrees=list(self.assert_deg), draws=self.draws, redraws=self.redraws,
                        probe=None, free_cols=list(self.cols))
        return cfg


def _assert_leaf(g):
    """a non-slot operand to assert: CONST zero often enough to be covered"""
    return g.const(0) if g.rng.random() < 0.12 else g.leaf()


def free(rng, nslots, nops, width=3, prep_width=0):
    """an arbitrary program of about nops ops: no trace satisfies it, which is
    intended -- check reports and quotient values are defined pointwise"""
    g = _Gen(rng, width, nslots, prep_width)
    if nslots == 0:
        for _ in range(nops):
            g.assert_zero(_assert_leaf(g))
        return g.build("free")
    while len(g.ops) < nops - 1:
        x = rng.random()
        if x < 0.16:
            w = g.written()
            g.assert_zero(rng.choice(w) if w and rng.random() < 0.6 else _assert_leaf(g))
        elif x < 0.20 and len(g.ops) + 20 < nops:
            g.chain()
        elif x < 0.24 and nslots >= 2 and len(g.ops) + 6 < nops:
            g.assert_zero(g.pow9())
        else:
            g.random_op()
    w = g.written()
    g.assert_zero(rng.choice(w) if w else _assert_leaf(g))
    return g.build("free")


def identity(rng, nslots, nasserts, width=3, prep_width=0):
    """every assert is E - E' with E' the same polynomial associated or expanded
    differently: 0 mod r for every input, reached as different multiples of r"""
    g = _Gen(rng, width, nslots, prep_width)
    top = True  # the first assert uses the highest slot: the register file is sized for it
    for _ in range(nasserts):
        if nslots == 0:
            g.assert_zero(g.const(0))
            continue
        S = rng.sample(range(nslots), min(nslots, 3))
        if top:
            S[0], top = nslots - 1, False
            S = S[:1] + [s for s in S[1:] if s != S[0]]
        a, b, c, d = (g.leaf() for _ in range(4))
        zero = g.const(0)
        if len(S) >= 3 and rng.random() < 0.4:
            # a composite operand: a raw product or a sum kept in the third slot
            g.must(rng.choice([MUL, ADD, SUB]), S[2], g.leaf(), g.leaf())
            a = S[2]
        s0 = S[0]
        t = rng.randrange(11 if len(S) >= 2 else 4)
        if t == 0:      # x - x
            if kind(a) != SLOT and rng.random() < 0.5:
                g.must(MUL, s0, a, b)
                g.must(SUB, s0, s0, s0)
            else:
                g.must(SUB, s0, a, a)
        elif t == 1:    # 0 x: a product asserted directly
            g.must(MUL, s0, *rng.sample([zero, a], 2))
        elif t == 2:    # x + (0 - x)
            g.must(SUB, s0, zero, a)
            g.must(ADD, s0, *rng.sample([a, s0], 2))
        elif t == 3:    # (a + b) - (b + a) in one slot: a + b - b - a
            g.must(ADD, s0, a, b)
            g.must(SUB, s0, s0, b)
            g.must(SUB, s0, s0, a)
        else:
            s1 = S[1]
            if t == 4:      # (a + b) c = a c + b c
                g.must(ADD, s0, a, b)
                g.must(MUL, s0, s0, c)
                g.must(MUL, s1, a, c)
                g.must(SUB, s0, s0, s1)
                g.must(MUL, s1, b, c)
                g.must(SUB, s0, s0, s1)
            elif t == 5:    # (a - b)(a + b) = a a - b b
                g.must(SUB, s0, a, b)
                g.must(ADD, s1, a, b)
                g.must(MUL, s0, s0, s1)
                g.must(MUL, s1, a, a)
                g.must(SUB, s0, s0, s1)
                g.must(MUL, s1, b, b)
                g.must(ADD, s0, s0, s1)
            elif t == 6:    # a b = b a
                g.must(MUL, s0, a, b)
                g.must(MUL, s1, b, a)
                g.must(SUB, s0, s0, s1)
            elif t == 7:    # (a b) c = a (b c)
                g.must(MUL, s0, a, b)
                g.must(MUL, s0, s0, c)
                g.must(MUL, s1, b, c)
                g.must(MUL, s1, a, s1)
                g.must(SUB, s0, s1, s0)
            elif t == 8:    # (a b)(c d) = (a c)(b d): raw products multiplied
                if len(S) < 3 or a == S[2]:
                    a = g.leaf()
                s2 = S[2] if len(S) >= 3 else None
                g.must(MUL, s0, a, b)
                g.must(MUL, s1, c, d)
                g.must(MUL, s0, s0, s1)
                if s2 is None:  # ((a c) b) d in one slot
                    g.must(MUL, s1, a, c)
                    g.must(MUL, s1, s1, b)
                    g.must(MUL, s1, s1, d)
                else:
                    g.must(MUL, s1, a, c)
                    g.must(MUL, s2, b, d)
                    g.must(MUL, s1, s1, s2)
                g.must(SUB, s0, s0, s1)
            elif t == 9:    # x^9 by squarings against x^9 by a chain (x a leaf)
                x = b
                g.must(MUL, s0, x, x)
                g.must(MUL, s0, s0, s0)
                g.must(MUL, s0, s0, s0)
                g.must(MUL, s0, s0, x)
                g.must(MUL, s1, x, x)
                for _ in range(2):
                    g.must(MUL, s1, s1, x)
                g.must(MUL, s1, s1, s1)     # x^8
                g.must(MUL, s1, x, s1)
                g.must(SUB, s0, s0, s1)
            else:           # sum of n products forwards = backwards (n >= 9: a long chain)
                n = rng.randint(9, 12)
                terms = [(g.leaf(), g.leaf()) for _ in range(n)]
                for i, (x, y) in enumerate(terms):
                    g.must(MUL, s1 if i else s0, x, y)
                    if i:
                        g.must(ADD, s0, s0, s1)
                for x, y in reversed(terms):
                    g.must(MUL, s1, y, x)
                    g.must(SUB, s0, s0, s1)
        # the zero times something, asserted as the raw product it is: a zero that
        # stands as a multiple of r, multiplied (a draw past degree 9 is dropped)
        x = rng.random()
        if x < 0.3:
            g.op(MUL, s0, *rng.sample([s0, g.leaf()], 2))
        elif x < 0.45 and len(S) >= 2:
            g.must(MUL, S[1], g.leaf(), g.leaf())
            g.op(MUL, s0, *rng.sample([s0, S[1]], 2))
        g.assert_zero(s0)
    return g.build("identity")


def solvable(rng, nslots, nasserts, nfree=2, prep_width=0, burst=6):
    """each assert is [selector *] (E - local[w - 1 - j]) with E over the first
    nfree columns (local and next), public values, constants and preprocessed
    cells: fill() computes the defined columns, so the trace satisfies the AIR"""
    width = nfree + nasserts
    kinds = [LOCAL, NEXT, LOCAL, NEXT, PUBLIC, CONST] + ([PREP_LOCAL, PREP_NEXT] if prep_width else [])
    g = _Gen(rng, width, nslots, prep_width, cols=list(range(nfree)), kinds=kinds)
    probe = []   # the same ops with E asserted in place of the difference
    for j in range(nasserts):
        col = LOCAL << 24 | (width - 1 - j)
        if nslots == 0:          # only a leaf can be asserted: the column is zero
            g.assert_zero(col)
            continue
        n0 = len(g.ops)
        for _ in range(rng.randint(1, burst)):
            g.random_op(MAX_DEG - 1)  # a selector may still multiply the difference
        e = rng.choice(g.written())
        probe += g.ops[n0:] + [(ASSERT, 0, e, 0)]
        n1 = len(g.ops)
        d = rng.randrange(nslots)
        g.must(SUB, d, *((e, col) if rng.random() < 0.5 else (col, e)))
        x = rng.random()
        if x < 0.6:
            sel = rng.choice([FIRST, LAST, TRANS]) << 24
            g.must(MUL, d, *rng.sample([sel, d], 2))
        probe += g.ops[n1:]
        g.assert_zero(d)
        g.deg[d] = None  # the difference is not an E: never read again
    cfg = g.build("solvable")
    if nslots:
        cfg.fuzz["probe"] = AirProgramConfig(width, nslots, list(g.consts), probe, prep_width=prep_width)
    return cfg


# ------------------------------------------------------------------ classes
FORMS = ["dst_is_operand", "dst_is_both_operands", "same_slot_twice", "same_cell_twice", "const_op_const",
         "selector_op_selector", "assert_raw_mul", "assert_local", "assert_next", "assert_public",
         "assert_const_zero", "assert_const_nonzero", "assert_first", "assert_last", "assert_trans",
         "overwritten_then_read", "sub_raw_product", "sub_selector", "mul_raw_raw", "degree_9", "addsub_chain_8"]
REGIMES = ["nslots_0", "nslots_1_5", "nslots_6_8", "nslots_9_16"]


def classes(cfg):
    """the op forms of FORMS a program holds, its nslots regime, and
    assert_kind_K / mul_kind_K for every operand kind K asserted / multiplied"""
    out = {regime(cfg.nslots)}
    raw, writes, deg = [False] * 16, [0] * 16, [0] * 16
    chain = [(0, False)] * 16   # (ADD / SUB ops in a row behind the slot, a product among their operands)

    def dg(x):
        return deg[x & 0xFFFFFF] if kind(x) == SLOT else LEAF_DEG[kind(x)]

    def is_raw(x):
        return kind(x) == SLOT and raw[x & 0xFFFFFF]

    sels = (FIRST, LAST, TRANS)
    for code, dst, a, b in cfg.ops:
        for x in (a,) if code == ASSERT else (a, b):
            if kind(x) == SLOT and writes[x & 0xFFFFFF] >= 2:
                out.add("overwritten_then_read")
        if code == ASSERT:
            k = kind(a)
            out.add(f"assert_kind_{k}")
            if is_raw(a):
                out.add("assert_raw_mul")
            names = {LOCAL: "assert_local", NEXT: "assert_next", PUBLIC: "assert_public", FIRST: "assert_first",
                     LAST: "assert_last", TRANS: "assert_trans"}
            if k in names:
                out.add(names[k])
            if k == CONST:
                out.add("assert_const_zero" if cfg.consts[a & 0xFFFFFF] == 0 else "assert_const_nonzero")
            continue
        sa, sb = a == dst and kind(a) == SLOT, b == dst and kind(b) == SLOT
        if sa or sb:
            out.add("dst_is_operand")
        if sa and sb:
            out.add("dst_is_both_operands")
        if a == b:
            out.add("same_slot_twice" if kind(a) == SLOT else "same_cell_twice" if kind(a) in
                    (LOCAL, NEXT, PREP_LOCAL, PREP_NEXT) else "same_other_twice")
        if kind(a) == CONST and kind(b) == CONST:
            out.add("const_op_const")
        if kind(a) in sels and kind(b) in sels:
            out.add("selector_op_selector")
        if code == SUB and is_raw(b):
            out.add("sub_raw_product")
        if code == SUB and kind(b) in sels:
            out.add("sub_selector")
        if code == MUL:
            out.update({f"mul_kind_{kind(a)}", f"mul_kind_{kind(b)}"})
            if is_raw(a) and is_raw(b):
                out.add("mul_raw_raw")
            d = dg(a) + dg(b)
            if d == MAX_DEG:
                out.add("degree_9")
            new = (0, False)
        else:
            d = max(dg(a), dg(b))
            ln = 1 + max([chain[x & 0xFFFFFF][0] for x in (a, b) if kind(x) == SLOT], default=0)
            pr = any(is_raw(x) or (kind(x) == SLOT and chain[x & 0xFFFFFF][1]) for x in (a, b))
            new = (ln, pr)
            if ln >= 8 and pr:
                out.add("addsub_chain_8")
        raw[dst], deg[dst], chain[dst] = code == MUL, d, new
        writes[dst] += 1
    return out


# ------------------------------------------------------------------- corpus
class Case:
    """one corpus entry: a LineaAIR of one or more configs; `parts` are the
    configs before shift(), ("perm", n) standing for a built-in permutation
    config of n + n columns"""

    def __init__(self, name, family, parts, seed):
        self.name, self.family, self.parts, self.seed = name, family, parts, seed
        cfgs, off = [], 0
        for p in parts:
            c = permutation_air(p[1]).configs[0] if isinstance(p, tuple) else copy.deepcopy(p)
            c.shift(off)
            off += c.width()
            cfgs.append(c)
        self.air = LineaAIR(cfgs)
        self.width = off
        progs = [p for p in parts if not isinstance(p, tuple)]
        self.prep_width = max(p.prep_width for p in progs)
        self.nslots = max(p.nslots for p in progs)
        self.programs = progs
        rng = random.Random(seed * 7919 + 1)
        self.extra = [draw_value(rng) for _ in range(NPUB - 2)]

    def __repr__(self):
        return self.name

    def degrees(self):
        """every constraint's tracked degree, in descriptor order"""
        out = []
        for p in self.parts:
            out += PR.program_degrees(permutation_air(p[1]).configs[0].to_program(), PD) if isinstance(p, tuple) \
                else p.fuzz["degrees"]
        return out

    def log_q(self):
        return (max(2, max(self.degrees())) - 2).bit_length()

    def prows(self, h, salt=0):
        if not self.prep_width:
            return None
        return draw_rows(random.Random(self.seed * 104729 + 31 * h + salt + 5), h, self.prep_width)

    def rows(self, h, pubi, perm_rows=None, salt=0):
        """an h-row trace: random edge-laden cells; the defined columns of a
        solvable program filled from the evaluator (next cyclic, as in the
        check); perm_rows: the rows of a valid permutation trace for the
        built-in config (random cells otherwise)"""
        rng = random.Random(self.seed * 1000003 + 17 * h + salt)
        prows = self.prows(h, salt)
        out = [[] for _ in range(h)]
        for p in self.parts:
            if isinstance(p, tuple):
                part = perm_rows if perm_rows is not None else draw_rows(rng, h, 2 * p[1] + 2)
            else:
                part = draw_rows(rng, h, p.desc_width)
                if p.fuzz["family"] == "solvable":
                    fill(p, part, pubi, prows)
            for i in range(h):
                out[i] += list(part[i])
        return out


def fill(cfg, rows, pubi, prows=None):
    """write the defined columns of a solvable program into rows (in place)"""
    h, w = len(rows), cfg.desc_width
    nfree = len(cfg.fuzz["free_cols"])
    for r in rows:
        r[nfree:] = [0] * (w - nfree)
    probe = cfg.fuzz["probe"]
    if probe is None:
        return
    p = prows if prows is not None else [None] * h
    for i in range(h):
        n = (i + 1) % h
        v = PR.eval_program(probe, rows[i], rows[n], pubi, 0, 0, 0, p[i], p[n])
        for j, x in enumerate(v):
            rows[i][w - 1 - j] = x


FREE_SLOTS = [0, 1, 2, 3, 5, 6, 7, 8, 9, 12, 16, 4, 16, 8, 2]
FREE_OPS = [1, 3, 10, 30, 60, 120, 200, 45, 90]


def _corpus():
    out = []
    for i in range(60):
        seed = 1000 + i
        rng = random.Random(seed)
        nslots, nops = FREE_SLOTS[i % len(FREE_SLOTS)], FREE_OPS[i % len(FREE_OPS)]
        wp = (0, 0, 1, 3)[i % 4]
        out.append(Case(f"free{i}", "free", [free(rng, nslots, nops, rng.randint(1, 6), wp)], seed))
    for i in range(30):
        seed = 2000 + i
        rng = random.Random(seed)
        nslots = [0, 1, 2, 3, 5, 6, 8, 9, 13, 16][i % 10]
        wp = (0, 3, 0, 1)[i % 4]
        out.append(Case(f"identity{i}", "identity", [identity(rng, nslots, rng.randint(1, 12), rng.randint(1, 5), wp)],
                        seed))
    for i in range(20):
        seed = 3000 + i
        rng = random.Random(seed)
        nslots = [1, 2, 4, 6, 8, 9, 16, 0, 3, 12][i % 10]
        wp = (0, 1, 0, 3, 0)[i % 5]
        out.append(Case(f"solvable{i}", "solvable",
                        [solvable(rng, nslots, rng.randint(1, 5), rng.randint(1, 3), wp, burst=rng.choice([3, 6, 12]))],
                        seed))
    # multi-config descriptors: the register file is sized by the largest nslots
    # (16 behind a 2-slot program), the constants of each program are its own
    for i, (slots, n) in enumerate([((2, 16, 0), 1), ((3, 9, 0), 2)]):
        seed = 4000 + i
        rng = random.Random(seed)
        a, b, c = (solvable(rng, s, rng.randint(1, 3), 2) for s in slots)
        out.append(Case(f"multi{i}", "solvable", [a, ("perm", n), b, c], seed))
    rng = random.Random(4100)
    a, b = solvable(rng, 4, 2, 2, burst=12), solvable(rng, 7, 3, 1, burst=3)
    assert len(a.consts) != len(b.consts), (len(a.consts), len(b.consts))
    out.append(Case("nconst0", "solvable", [a, b], 4100))
    rng = random.Random(4102)
    a, b = identity(rng, 5, 6, 2), free(rng, 11, 40, 3)
    assert len(a.consts) != len(b.consts), (len(a.consts), len(b.consts))
    out.append(Case("nconst1", "free", [a, b], 4102))
    return out


_CORPUS = None


def corpus():
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = _corpus()
    return _CORPUS


def large_subset():
    """12 cases spanning the four regimes (the longest program of at most 130
    ops of each family in each) and the first multi-config descriptor, for the
    larger heights"""
    out = []
    for reg in REGIMES:
        for fam in ("free", "identity", "solvable"):
            c = [x for x in corpus() if len(x.parts) == 1 and x.family == fam and regime(x.nslots) == reg
                 and len(x.programs[0].ops) <= 130]
            out.append(max(c, key=lambda x: len(x.programs[0].ops)))
    return out + [x for x in corpus() if x.name == "multi0"]


# ----------------------------------------------------------------- references
def report(air, rows, pubi, cap, prows=None):
    """the check's report from the big-integer evaluator (built-in configs
    through their restatement as programs)"""
    return PR.report(lower(air), rows, pubi, cap, prows)


def quotient_ref(air, ev_rows, h, log_q, pubi, alpha, prows=None):
    """the quotient's values on GEN * <w_Q>, Q = h << log_q, natural order, as
    ints: every constraint from the big-integer evaluator on rows i N / Q and
    i N / Q + N / h of ev_rows (N rows: the columns on GEN * <w_N>, natural
    order; prows: the preprocessed matrix likewise), folded by alpha and
    divided by Z_H"""
    N = len(ev_rows)
    log_h = h.bit_length() - 1
    Q = h << log_q
    step = N // Q
    low = lower(air)
    whinv = pow(two_adic_generator(log_h), R - 2, R)
    wq = two_adic_generator(log_h + log_q)
    p = prows if prows is not None else [None] * N
    out = []
    for i in range(Q):
        x = GENERATOR * pow(wq, i, R) % R
        zh = (pow(x, h, R) - 1) % R
        first = zh * pow(x - 1, R - 2, R) % R
        last = zh * pow(x - whinv, R - 2, R) % R
        n = (i * step + N // h) % N
        cons = PR.eval_air(low, ev_rows[i * step], ev_rows[n], pubi, first, last, (x - whinv) % R, p[i * step], p[n])
        acc = 0
        for c in cons:
            acc = (acc * alpha + c) % R
        out.append(acc * pow(zh, R - 2, R) % R)
    return out


def brev(x, bits):
    return int(format(x, f"0{bits}b")[::-1], 2) if bits else 0


def to_matrix(rows):
    h, w = len(rows), len(rows[0])
    return to_mont([x for r in rows for x in r]).reshape(h, w, 4)


def to_lde(ev_rows):
    """the N x w limb matrix in the bit-reversed row order the prover keeps an LDE in"""
    N = len(ev_rows)
    bits = N.bit_length() - 1
    m = to_matrix(ev_rows)
    idx = [brev(n, bits) for n in range(N)]
    out = m.copy()
    out[idx] = m
    return out
