"""AIR configs of the reference's ``air`` crate, encoded for the GPU quotient.

Mirrors ``AirPermutationConfig`` (air/src/air_permutation.rs:1-24),
``AirLookupConfig`` (air/src/air_lookup.rs:1-40), ``AirConfig`` and
``LineaAIR`` (air/src/lib.rs:11-54).  ``LineaAIR.descriptor()`` produces the
int32 descriptor of include/lsp.h that the quotient kernel interprets with
the constraint order of ``LineaAIR::eval`` (air/src/lib.rs:47-167).
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple, Union

from .field import MODULUS

LSP_AIR_PERMUTATION, LSP_AIR_LOOKUP, LSP_AIR_PROGRAM, LSP_AIR_PROGRAM_PREP = 1, 2, 3, 4


@dataclass
class AirPermutationConfig:
    a_columns_ids: List[int]
    b_columns_ids: List[int]
    b_inverse_id: int
    check_id: int

    @staticmethod
    def block(na: int, nb: int, col0: int = 0) -> "AirPermutationConfig":
        """A witness block's config, its first column ``col0``: a.., b.., b_inverse,
        check (trace/src/permutation.rs:81-90; csrc/witness_layout.hpp's PermBlock)."""
        ids = itertools.count(col0)
        return AirPermutationConfig([next(ids) for _ in range(na)], [next(ids) for _ in range(nb)], next(ids),
                                    next(ids))

    def shift(self, shift: int) -> None:
        self.a_columns_ids = [i + shift for i in self.a_columns_ids]
        self.b_columns_ids = [i + shift for i in self.b_columns_ids]
        self.b_inverse_id += shift
        self.check_id += shift

    def width(self) -> int:
        return len(self.a_columns_ids) + len(self.b_columns_ids) + 2

    def to_program(self) -> "AirProgramConfig":
        """The same constraints (air/src/lib.rs:116-167, in eval's order) as an
        ``AirProgramConfig``: field arithmetic is exact, so the proof bytes are
        those of this config."""
        b = ProgramBuilder(max(self.a_columns_ids + self.b_columns_ids + [self.b_inverse_id, self.check_id]) + 1)
        loc, nxt = b.local, b.next
        a_l, b_l = _challenge(b, loc, self.a_columns_ids), _challenge(b, loc, self.b_columns_ids)
        b.assert_zero(b_l * loc[self.b_inverse_id] - 1, "b_inverse")
        b.when_first_row().assert_zero(loc[self.check_id] - a_l * loc[self.b_inverse_id], "first_row")
        a_n = _challenge(b, nxt, self.a_columns_ids)
        b.when_transition().assert_zero(
            nxt[self.check_id] - loc[self.check_id] * a_n * nxt[self.b_inverse_id], "transition")
        b.when_last_row().assert_zero(loc[self.check_id] - 1, "last_row")
        return b.build(ncols=self.width())

    def encode(self) -> List[int]:
        return ([LSP_AIR_PERMUTATION, len(self.a_columns_ids), len(self.b_columns_ids)]
                + list(self.a_columns_ids) + list(self.b_columns_ids) + [self.b_inverse_id, self.check_id])


@dataclass
class AirLookupConfig:
    a_columns_ids: List[int]
    b_columns_ids: List[List[int]]
    a_filter_id: int
    b_filter_id: List[int]
    a_inverses_id: int
    b_inverses_id: List[int]
    occurrences_id: List[int]
    check_id: int

    @staticmethod
    def block(na: int, nt: int, nbc: int, col0: int = 0) -> "AirLookupConfig":
        """A witness block's config, its first column ``col0``: a.., tables.., a_filter,
        b_filters.., a_inverse, b_inverses.., multiplicities.., sum
        (trace/src/lookup.rs:178-214; csrc/witness_layout.hpp's LookupBlock)."""
        ids = itertools.count(col0)

        def take(k):
            return [next(ids) for _ in range(k)]

        return AirLookupConfig(take(na), [take(nbc) for _ in range(nt)], next(ids), take(nt), next(ids), take(nt),
                               take(nt), next(ids))

    def shift(self, shift: int) -> None:
        self.a_columns_ids = [i + shift for i in self.a_columns_ids]
        self.b_columns_ids = [[i + shift for i in t] for t in self.b_columns_ids]
        self.a_filter_id += shift
        self.b_filter_id = [i + shift for i in self.b_filter_id]
        self.a_inverses_id += shift
        self.b_inverses_id = [i + shift for i in self.b_inverses_id]
        self.occurrences_id = [i + shift for i in self.occurrences_id]
        self.check_id += shift

    def width(self) -> int:
        return len(self.a_columns_ids) + len(self.b_columns_ids) * (len(self.b_columns_ids[0]) + 3) + 3

    def to_program(self) -> "AirProgramConfig":
        """The same constraints (air/src/lib.rs:57-114, in eval's order) as an
        ``AirProgramConfig``; see ``AirPermutationConfig.to_program``."""
        cols = (self.a_columns_ids + [i for t in self.b_columns_ids for i in t] + self.b_filter_id
                + self.b_inverses_id + self.occurrences_id + [self.a_filter_id, self.a_inverses_id, self.check_id])
        b = ProgramBuilder(max(cols) + 1)
        loc, nxt = b.local, b.next
        b.assert_zero(_challenge(b, loc, self.a_columns_ids) * loc[self.a_inverses_id] - 1, "a_inverse")
        lc = loc[self.a_filter_id] * loc[self.a_inverses_id]
        nc = nxt[self.a_filter_id] * nxt[self.a_inverses_id]
        for t, ids in enumerate(self.b_columns_ids):
            bf, bi, oc = self.b_filter_id[t], self.b_inverses_id[t], self.occurrences_id[t]
            b.assert_zero(_challenge(b, loc, ids) * loc[bi] - 1, f"b_inverse[{t}]")
            lc = lc - loc[bf] * loc[oc] * loc[bi]
            nc = nc - nxt[bf] * nxt[oc] * nxt[bi]
        b.when_first_row().assert_zero(loc[self.check_id] - lc, "first_row")
        b.when_transition().assert_zero(nxt[self.check_id] - loc[self.check_id] - nc, "transition")
        b.when_last_row().assert_zero(loc[self.check_id], "last_row")
        return b.build(ncols=self.width())

    def encode(self) -> List[int]:
        nt, nbc = len(self.b_columns_ids), len(self.b_columns_ids[0])
        out = [LSP_AIR_LOOKUP, len(self.a_columns_ids)] + list(self.a_columns_ids) + [nt, nbc]
        for t in self.b_columns_ids:
            assert len(t) == nbc, "all B tables must have the same number of columns"
            out += list(t)
        return (out + [self.a_filter_id] + list(self.b_filter_id) + [self.a_inverses_id]
                + list(self.b_inverses_id) + list(self.occurrences_id) + [self.check_id])


# ---------------------------------------------------------------- programs
# LSP_AIR_PROGRAM (include/lsp.h): operand kinds and opcodes
(OPND_SLOT, OPND_LOCAL, OPND_NEXT, OPND_PUBLIC, OPND_CONST, OPND_FIRST, OPND_LAST, OPND_TRANS) = range(8)
OPND_PREP_LOCAL, OPND_PREP_NEXT = 8, 9  # LSP_AIR_PROGRAM_PREP only: a cell of the preprocessed matrix
OP_ADD, OP_SUB, OP_MUL, OP_ASSERT_ZERO = 1, 2, 3, 4
MAX_SLOTS = 16


def _i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


@dataclass
class AirProgramConfig:
    """An LSP_AIR_PROGRAM config in its encoded form: ``ops`` are (opcode, dst,
    a, b) with operands ``kind << 24 | payload``, ``consts`` canonical ints.
    ``desc_width`` bounds the (absolute) column ids; ``ncols`` is what the
    config adds to ``LineaAIR.width``.  ``prep_width`` > 0: the program reads
    that many preprocessed columns (operand kinds 8 and 9) and encodes as
    LSP_AIR_PROGRAM_PREP; 0 encodes as LSP_AIR_PROGRAM, exactly as before."""
    desc_width: int
    nslots: int
    consts: List[int]
    ops: List[Tuple[int, int, int, int]]
    ncols: int = -1
    labels: Optional[List[Optional[str]]] = field(default=None, compare=False)
    prep_width: int = 0

    def __post_init__(self):
        if self.ncols < 0:
            self.ncols = self.desc_width

    @property
    def nassert(self) -> int:
        return sum(1 for o in self.ops if o[0] == OP_ASSERT_ZERO)

    def shift(self, shift: int) -> None:
        def sh(x):
            return x + shift if (x >> 24) in (OPND_LOCAL, OPND_NEXT) else x
        self.ops = [(c, d, sh(a), sh(b) if c != OP_ASSERT_ZERO else b) for c, d, a, b in self.ops]
        self.desc_width += shift

    def width(self) -> int:
        return self.ncols

    def encode(self) -> List[int]:
        head = [LSP_AIR_PROGRAM_PREP, self.desc_width, self.prep_width] if self.prep_width else \
            [LSP_AIR_PROGRAM, self.desc_width]
        out = head + [self.nslots, len(self.consts), len(self.ops), self.nassert]
        for c in self.consts:
            out += [_i32(c >> (32 * k)) for k in range(8)]
        for o in self.ops:
            out += [_i32(x) for x in o]
        return out

    def names(self) -> List[str]:
        lab = self.labels or []
        return [lab[i] if i < len(lab) and lab[i] else f"assert[{i}]" for i in range(self.nassert)]


class Expr:
    """A node of a ``ProgramBuilder``'s expression graph; ``+ - *`` and unary
    ``-`` with other expressions or integer constants."""
    __slots__ = ("b", "id")

    def __init__(self, b: "ProgramBuilder", nid: int):
        self.b, self.id = b, nid

    def _bin(self, op, x, y):
        return Expr(self.b, self.b._node(op, self.b._lift(x), self.b._lift(y)))

    def __add__(self, o): return self._bin(OP_ADD, self, o)
    def __radd__(self, o): return self._bin(OP_ADD, o, self)
    def __sub__(self, o): return self._bin(OP_SUB, self, o)
    def __rsub__(self, o): return self._bin(OP_SUB, o, self)
    def __mul__(self, o): return self._bin(OP_MUL, self, o)
    def __rmul__(self, o): return self._bin(OP_MUL, o, self)
    def __neg__(self): return self._bin(OP_SUB, 0, self)


class _Vars:
    def __init__(self, b, kind, n):
        self.b, self.kind, self.n = b, kind, n

    def __getitem__(self, i: int) -> Expr:
        if not 0 <= i < self.n:
            raise IndexError(f"index {i} outside [0, {self.n})")
        return Expr(self.b, self.b._node(self.kind, i, 0))


class _When:
    def __init__(self, b, sel: Expr):
        self.b, self.sel = b, sel

    def assert_zero(self, e, label: Optional[str] = None):
        self.b.assert_zero(self.sel * e, label)

    def assert_eq(self, x, y, label: Optional[str] = None):
        self.b.assert_zero(self.sel * (self.b._expr(x) - y), label)


class ProgramBuilder:
    """Constraints stated in the shape of p3's ``AirBuilder``::

        b = ProgramBuilder(2)
        b.when_first_row().assert_eq(b.local[0], b.public[2])
        b.when_transition().assert_eq(b.next[1], b.local[0] + b.local[1])
        cfg = b.build()

    ``ProgramBuilder(width, preprocessed_width=wp)`` also has
    ``b.preprocessed[i]`` and ``b.preprocessed_next[i]``, the cells of the wp
    fixed columns (p3's ``PairBuilder::preprocessed()``) in the rows of
    ``local`` and ``next``; such a program encodes as LSP_AIR_PROGRAM_PREP.

    Equal subexpressions are one node (hash-consing: common-subexpression
    elimination), constants with constants are folded mod r.  ``build()``
    orders each expression so that the side needing more slots runs first
    (Sethi-Ullman), keeps a shared node in its slot until its last use and
    raises ``ValueError`` when more than 16 slots would be live."""

    def __init__(self, width: int, preprocessed_width: int = 0):
        if not 1 <= width <= 1 << 20:
            raise ValueError("width outside [1, 2^20]")
        if not 0 <= preprocessed_width <= 1 << 20:
            raise ValueError("preprocessed_width outside [0, 2^20]")
        self.width = width
        self.preprocessed_width = preprocessed_width
        self._nodes: List[Tuple[int, int, int]] = []   # leaves: (-kind - 1, payload, 0); ops: (opcode, a, b)
        self._ids: Dict[Tuple[int, int, int], int] = {}
        self._asserts: List[Tuple[int, Optional[str]]] = []
        self.local = _Vars(self, -OPND_LOCAL - 1, width)
        self.next = _Vars(self, -OPND_NEXT - 1, width)
        self.public = _Vars(self, -OPND_PUBLIC - 1, 1 << 16)
        self.preprocessed = _Vars(self, -OPND_PREP_LOCAL - 1, preprocessed_width)
        self.preprocessed_next = _Vars(self, -OPND_PREP_NEXT - 1, preprocessed_width)
        self.is_first_row = Expr(self, self._node(-OPND_FIRST - 1, 0, 0))
        self.is_last_row = Expr(self, self._node(-OPND_LAST - 1, 0, 0))
        self.is_transition = Expr(self, self._node(-OPND_TRANS - 1, 0, 0))

    def _node(self, op, a, b) -> int:
        if op in (OP_ADD, OP_SUB, OP_MUL):
            x, y = self._nodes[a], self._nodes[b]
            if x[0] == -OPND_CONST - 1 and y[0] == -OPND_CONST - 1:
                v = x[1] + y[1] if op == OP_ADD else x[1] - y[1] if op == OP_SUB else x[1] * y[1]
                return self._node(-OPND_CONST - 1, v % MODULUS, 0)
        key = (op, a, b)
        nid = self._ids.get(key)
        if nid is None:
            nid = self._ids[key] = len(self._nodes)
            self._nodes.append(key)
        return nid

    def _lift(self, x) -> int:
        if isinstance(x, Expr):
            if x.b is not self:
                raise ValueError("expression of another builder")
            return x.id
        if isinstance(x, int):
            return self._node(-OPND_CONST - 1, x % MODULUS, 0)
        raise TypeError(f"cannot use {type(x).__name__} in a constraint")

    def _expr(self, x) -> Expr:
        return Expr(self, self._lift(x))

    def const(self, v: int) -> Expr:
        return self._expr(int(v))

    def when_first_row(self) -> _When: return _When(self, self.is_first_row)
    def when_last_row(self) -> _When: return _When(self, self.is_last_row)
    def when_transition(self) -> _When: return _When(self, self.is_transition)

    def assert_zero(self, e, label: Optional[str] = None) -> None:
        self._asserts.append((self._lift(e), label))

    def assert_eq(self, x, y, label: Optional[str] = None) -> None:
        self.assert_zero(self._expr(x) - y, label)

    def build(self, ncols: int = -1) -> AirProgramConfig:
        if not self._asserts:
            raise ValueError("a program needs at least one assert")
        nodes = self._nodes
        is_op = [n[0] > 0 for n in nodes]
        # reachable nodes, uses per node (one per referencing edge and per assert),
        # and the Sethi-Ullman need: a leaf is an operand and needs no slot
        uses = [0] * len(nodes)
        seen = [False] * len(nodes)
        order = []
        for root, _ in self._asserts:
            uses[root] += 1
            st = [root]
            while st:
                n = st.pop()
                if seen[n] or not is_op[n]:
                    continue
                seen[n] = True
                order.append(n)
                for c in nodes[n][1:]:
                    uses[c] += 1
                    st.append(c)
        need = [0] * len(nodes)
        for n in sorted(order):  # a node's operands have lower ids
            x, y = need[nodes[n][1]], need[nodes[n][2]]
            need[n] = max(1, x + 1 if x == y else max(x, y))
        consts: Dict[int, int] = {}
        ops: List[Tuple[int, int, int, int]] = []
        slot_of: Dict[int, int] = {}
        free = list(range(MAX_SLOTS - 1, -1, -1))  # lowest on top
        top = 0

        def operand(n):
            if is_op[n]:
                return OPND_SLOT << 24 | slot_of[n]
            kind, v = -nodes[n][0] - 1, nodes[n][1]
            if kind == OPND_CONST:
                v = consts.setdefault(v, len(consts))
                if v >= 1 << 16:
                    raise ValueError("a program holds at most 2^16 constants")
            return kind << 24 | v

        def release(n):
            uses[n] -= 1
            if is_op[n] and uses[n] == 0:
                free.append(slot_of.pop(n))
                free.sort(reverse=True)

        for root, _ in self._asserts:
            st = [(root, 0)]
            while st:
                n, phase = st.pop()
                if not is_op[n] or n in slot_of:
                    continue
                op, a, b = nodes[n]
                if phase == 0:
                    st.append((n, 1))
                    first, second = (a, b) if need[a] >= need[b] else (b, a)
                    st.append((second, 0))
                    st.append((first, 0))
                    continue
                oa, ob = operand(a), operand(b)
                release(a)
                release(b)
                if not free:
                    raise ValueError(f"the program needs more than {MAX_SLOTS} slots: too many values are live "
                                     "at once (restate the constraints so that shared values are used sooner)")
                s = free.pop()
                top = max(top, s + 1)
                slot_of[n] = s
                ops.append((op, s, oa, ob))
            ops.append((OP_ASSERT_ZERO, 0, operand(root), 0))
            release(root)
        if len(ops) > 1 << 20:
            raise ValueError("a program holds at most 2^20 ops")
        cl = [0] * len(consts)
        for v, i in consts.items():
            cl[i] = v
        return AirProgramConfig(self.width, top, cl, ops, ncols, [lab for _, lab in self._asserts],
                                self.preprocessed_width)


def _challenge(b: ProgramBuilder, row, ids) -> Expr:
    """alpha-Horner of a row's columns from ZERO, plus delta (air/src/lib.rs)"""
    acc = b.const(0)
    for k in ids:
        acc = acc * b.public[0] + row[k]
    return acc + b.public[1]


def decode_program(it, prep: bool = False) -> AirProgramConfig:
    """the words of an LSP_AIR_PROGRAM (prep: LSP_AIR_PROGRAM_PREP) config after its type word"""
    width = next(it)
    prep_width = next(it) if prep else 0
    nslots, nconst, nops, nassert = (next(it) for _ in range(4))
    consts = [sum((next(it) & 0xFFFFFFFF) << (32 * k) for k in range(8)) for _ in range(nconst)]
    ops = [tuple(next(it) & 0xFFFFFFFF if j >= 2 else next(it) for j in range(4)) for _ in range(nops)]
    cfg = AirProgramConfig(width, nslots, consts, ops, prep_width=prep_width)
    if cfg.nassert != nassert:
        raise ValueError("nassert is not the number of ASSERT_ZERO ops")
    return cfg


AirConfig = Union[AirLookupConfig, AirPermutationConfig, AirProgramConfig]


@dataclass
class LineaAIR:
    configs: List[AirConfig] = field(default_factory=list)

    @property
    def width(self) -> int:
        return sum(c.width() for c in self.configs)

    def descriptor(self) -> List[int]:
        out = [len(self.configs)]
        for c in self.configs:
            out += c.encode()
        return out

    def constraint_names(self) -> List[str]:
        """One name per constraint of ``LineaAIR::eval`` in its order (the
        indexing of ``lsp_air_constraint_info`` and of a ``ConstraintReport``),
        e.g. ``"cfg 2 lookup: b_inverse[1]"``, ``"cfg 5 permutation: transition"``."""
        out = []
        for k, c in enumerate(self.configs):
            if isinstance(c, AirProgramConfig):
                out += [f"cfg {k} program: {x}" for x in c.names()]
            elif isinstance(c, AirPermutationConfig):
                kinds = ["b_inverse", "first_row", "transition", "last_row"]
                out += [f"cfg {k} permutation: {x}" for x in kinds]
            else:
                kinds = (["a_inverse"] + [f"b_inverse[{t}]" for t in range(len(c.b_columns_ids))]
                         + ["first_row", "transition", "last_row"])
                out += [f"cfg {k} lookup: {x}" for x in kinds]
        return out

    @staticmethod
    def from_descriptor(d: List[int]) -> "LineaAIR":
        it = iter(d)
        n = next(it)
        cfgs: List[AirConfig] = []
        for _ in range(n):
            t = next(it)
            if t == LSP_AIR_PERMUTATION:
                na, nb = next(it), next(it)
                a = [next(it) for _ in range(na)]
                b = [next(it) for _ in range(nb)]
                cfgs.append(AirPermutationConfig(a, b, next(it), next(it)))
            elif t == LSP_AIR_LOOKUP:
                na = next(it)
                a = [next(it) for _ in range(na)]
                nt, nbc = next(it), next(it)
                b = [[next(it) for _ in range(nbc)] for _ in range(nt)]
                af = next(it)
                bf = [next(it) for _ in range(nt)]
                ai = next(it)
                bi = [next(it) for _ in range(nt)]
                oc = [next(it) for _ in range(nt)]
                cfgs.append(AirLookupConfig(a, b, af, bf, ai, bi, oc, next(it)))
            elif t == LSP_AIR_PROGRAM:
                cfgs.append(decode_program(it))
            elif t == LSP_AIR_PROGRAM_PREP:
                cfgs.append(decode_program(it, prep=True))
            else:
                raise ValueError(f"unknown AIR config type {t}")
        assert next(it, None) is None, "trailing data in AIR descriptor"
        return LineaAIR(cfgs)


def lower(air: LineaAIR, which=None) -> LineaAIR:
    """``air`` with its built-in configs restated as programs (``which``: the
    indices to lower, default all); the same constraints in the same order."""
    return LineaAIR([c.to_program() if not isinstance(c, AirProgramConfig) and (which is None or k in which) else c
                     for k, c in enumerate(air.configs)])


def permutation_air(ncols: int) -> LineaAIR:
    """The benchmark AIR: one permutation group of ncols 'from' + ncols 'to'
    columns (trace/src/permutation.rs:81-90 column layout)."""
    return LineaAIR([AirPermutationConfig.block(ncols, ncols)])
