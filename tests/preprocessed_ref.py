"""Shared by tests/test_preprocessed.py and tests/test_gpu_preprocessed.py: a
big-integer evaluator of programs that read preprocessed columns (operand kinds
8 PREP_LOCAL and 9 PREP_NEXT of LSP_AIR_PROGRAM_PREP), the check_constraints
report made from it, an independent prover for proofs over such AIRs (prove,
below), and four small AIRs, each in two equivalent layouts built by one
function from one constraint list (keys3 / keys5: three and five fixed columns):

  layout "a"   all wp + w columns in the main trace (fixed columns first), a
               type-3 program -- what the library could already do
  layout "b"   the first wp columns preprocessed, a type-4 program

Nothing here calls the library."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from linea_stark_prover_amd.air import LineaAIR, ProgramBuilder  # noqa: E402
from linea_stark_prover_amd.field import MODULUS, to_mont  # noqa: E402

R = MODULUS


# -------------------------------------------------------------- evaluator
def eval_program(cfg, loc, nxt, pub, first, last, trans, ploc=None, pnxt=None):
    """every ASSERT_ZERO's value mod r, in order, as Python ints"""
    slot = [None] * 16
    out = []

    def opnd(x):
        kind, v = x >> 24, x & 0xFFFFFF
        if kind == 0:
            assert slot[v] is not None, "slot read before it is written"
            return slot[v]
        if kind in (8, 9):
            assert cfg.prep_width and v < cfg.prep_width, "preprocessed column outside prep_width"
            return (ploc if kind == 8 else pnxt)[v]
        return {1: lambda: loc[v], 2: lambda: nxt[v], 3: lambda: pub[v], 4: lambda: cfg.consts[v],
                5: lambda: first, 6: lambda: last, 7: lambda: trans}[kind]()

    for code, dst, a, b in cfg.ops:
        if code == 4:
            out.append(opnd(a) % R)
        else:
            x, y = opnd(a), opnd(b)
            slot[dst] = (x + y if code == 1 else x - y if code == 2 else x * y) % R
    return out


def eval_air(air, loc, nxt, pub, first, last, trans, ploc=None, pnxt=None):
    out = []
    for c in air.configs:
        out += eval_program(c, loc, nxt, pub, first, last, trans, ploc, pnxt)
    return out


def program_degrees(cfg, pd):
    """main and preprocessed variables 1, constant 0, public pd, first / last
    selector 1, transition selector 0; Add / Sub max, Mul sum -- per assert"""
    slot = [0] * 16
    leaf = {1: 1, 2: 1, 3: pd, 4: 0, 5: 1, 6: 1, 7: 0, 8: 1, 9: 1}
    out = []

    def deg(x):
        return slot[x & 0xFFFFFF] if x >> 24 == 0 else leaf[x >> 24]

    for code, dst, a, b in cfg.ops:
        if code == 4:
            out.append(deg(a))
        else:
            slot[dst] = deg(a) + deg(b) if code == 3 else max(deg(a), deg(b))
    return out


def report(air, rows, pub, cap, prows=None):
    """tests/check_constraints_ref.py oracle_report's shape, from eval_air;
    prows: the rows of the preprocessed matrix"""
    h = len(rows)
    p = prows if prows is not None else [None] * h
    ncons = sum(c.nassert for c in air.configs)
    counts, first_rows, details, failed = [0] * ncons, [None] * ncons, [], 0
    for i in range(h):
        n = (i + 1) % h
        v = eval_air(air, rows[i], rows[n], pub, int(i == 0), int(i == h - 1), int(i != h - 1), p[i], p[n])
        bad = [j for j in range(ncons) if v[j]]
        failed += bool(bad)
        for j in bad:
            counts[j] += 1
            if first_rows[j] is None:
                first_rows[j] = i
            if len(details) < cap:
                details.append((i, j, v[j]))
    first = None
    if failed:
        r = min(x for x in first_rows if x is not None)
        first = (r, min(j for j in range(ncons) if first_rows[j] == r))
    return dict(ok=failed == 0, failed_rows=failed, violations=sum(counts), first=first, counts=counts,
                first_rows=first_rows, details=details)


def to_matrix(rows):
    h, w = len(rows), len(rows[0])
    return to_mont([x for r in rows for x in r]).reshape(h, w, 4)


# ------------------------------------------------------------------- AIRs
# name -> (wp, w, constraints(b, fixed, fixed_next, main, main_next))
def _keyed(b, f, fn, m, mn):
    """x' = x^2 + k with a fixed key schedule k; x starts at public value 2.
    Degree 2: one quotient chunk."""
    b.when_first_row().assert_eq(m[0], b.public[2], "x starts at x0")
    b.when_transition().assert_eq(mn[0], m[0] * m[0] + f[0], "x' = x^2 + k")


def _gated(b, f, fn, m, mn):
    """x' = s (x^3 + k') + (1 - s) (x + k): a fixed selector s in {0, 1} picks
    the round, k' is the key of the next row (PREP_NEXT).  Degree 4: four chunks."""
    s, k, x = f[0], f[1], m[0]
    b.when_first_row().assert_eq(x, b.public[2], "x starts at x0")
    b.when_transition().assert_eq(mn[0], s * (x * x * x + fn[1]) + (1 - s) * (x + k), "gated round")


PRESSURE_N = 9


def _pressure(b, f, fn, m, mn):
    """the n = 9 products t_i = x_i k_i' (a main cell times the next row's
    fixed cell) are shared by a forward and a backward sum, so all of them stay
    in slots beside the first sum's accumulator: 10 live slots, the 128-thread
    block form.  Public value 2 is the sum's value."""
    n = PRESSURE_N
    t = [m[i] * fn[i] for i in range(n)]
    s = t[0]
    for x in t[1:]:
        s = s + x
    u = t[n - 1]
    for x in reversed(t[:n - 1]):
        u = u + x
    b.assert_eq(s, b.public[2], "forward sum")
    b.assert_eq(u + f[0], b.public[2] + f[0], "backward sum")


def _wide(b, f, fn, m, mn):
    """keyed with two more main columns (w = 3 > wp = 1): y' = y + x, z = x y"""
    b.when_first_row().assert_eq(m[0], b.public[2], "x starts at x0")
    b.when_transition().assert_eq(mn[0], m[0] * m[0] + f[0], "x' = x^2 + k")
    b.when_transition().assert_eq(mn[1], m[1] + m[0], "y' = y + x")
    b.assert_eq(m[2], m[0] * m[1], "z = x y")


def _keys(n):
    def constraints(b, f, fn, m, mn):
        """keyed with n fixed columns: x' = x^2 + k_0 + ... + k_(n-1)"""
        b.when_first_row().assert_eq(m[0], b.public[2], "x starts at x0")
        ks = f[0]
        for k in f[1:]:
            ks = ks + k
        b.when_transition().assert_eq(mn[0], m[0] * m[0] + ks, "x' = x^2 + sum k")
    return constraints


AIRS = {"keyed": (1, 1, _keyed), "gated": (2, 1, _gated), "pressure": (PRESSURE_N, PRESSURE_N, _pressure),
        "wide": (1, 3, _wide), "keys3": (3, 1, _keys(3)), "keys5": (5, 1, _keys(5))}
LOG_Q = {"keyed": 0, "gated": 2, "pressure": 0, "wide": 0, "keys3": 0, "keys5": 0}


def build_air(name, layout):
    wp, w, constraints = AIRS[name]
    if layout == "a":
        b = ProgramBuilder(wp + w)
        f, fn = [b.local[i] for i in range(wp)], [b.next[i] for i in range(wp)]
        m, mn = [b.local[wp + i] for i in range(w)], [b.next[wp + i] for i in range(w)]
    else:
        assert layout == "b"
        b = ProgramBuilder(w, preprocessed_width=wp)
        f, fn = [b.preprocessed[i] for i in range(wp)], [b.preprocessed_next[i] for i in range(wp)]
        m, mn = [b.local[i] for i in range(w)], [b.next[i] for i in range(w)]
    constraints(b, f, fn, m, mn)
    return LineaAIR([b.build()])


def build_rows(name, h, x0=5):
    """(fixed rows h x wp, main rows h x w, the public values after [alpha, delta])
    of a trace that satisfies the AIR"""
    if name == "keyed":
        fixed = [[(7 * j * j + 3) % R] for j in range(h)]
        main, x = [], x0
        for j in range(h):
            main.append([x])
            x = (x * x + fixed[j][0]) % R
        return fixed, main, [x0]
    if name.startswith("keys"):
        n = AIRS[name][0]
        fixed = [[(7 * j * j + 3 + 11 * i) % R for i in range(n)] for j in range(h)]
        main, x = [], x0
        for j in range(h):
            main.append([x])
            x = (x * x + sum(fixed[j])) % R
        return fixed, main, [x0]
    if name == "gated":
        fixed = [[int(j * 5 % 3 == 0), (R - 1 - j * j) % R] for j in range(h)]
        main, x = [], x0
        for j in range(h):
            main.append([x])
            s, k, kn = fixed[j][0], fixed[j][1], fixed[(j + 1) % h][1]
            x = (pow(x, 3, R) + kn) % R if s else (x + k) % R
        return fixed, main, [x0]
    if name == "wide":
        fixed = [[(7 * j * j + 3) % R] for j in range(h)]
        main, x, y = [], x0, 1
        for j in range(h):
            main.append([x, y, x * y % R])
            x, y = (x * x + fixed[j][0]) % R, (y + x) % R
        return fixed, main, [x0]
    assert name == "pressure" and h % 2 == 0
    n = PRESSURE_N
    # x_i = k_i = (i + 2) on even rows and -(i + 2) on odd ones: every product of a
    # row's main cell with its successor's fixed cell (cyclically) is -(i + 2)^2
    fixed = [[(i + 2) * (1 if j % 2 == 0 else -1) % R for i in range(n)] for j in range(h)]
    main = [list(r) for r in fixed]
    return fixed, main, [-sum((i + 2) ** 2 for i in range(n)) % R]


def keyed_sum(wp):
    """x' = x^2 + fixed[0] + ... + fixed[wp - 1] on one main column (layout b
    only), the sum running in the one slot that held x^2: the program reads
    every preprocessed column, so prep_width = wp at any width, and its
    register file stays one slot.  x starts at public value 2.  Degree 2."""
    b = ProgramBuilder(1, preprocessed_width=wp)
    x, s = b.local[0], b.local[0] * b.local[0]
    for i in range(wp):
        s = s + b.preprocessed[i]
    b.when_first_row().assert_eq(x, b.public[2], "x starts at x0")
    b.when_transition().assert_eq(b.next[0], s, "x' = x^2 + sum fixed")
    cfg = b.build()
    assert cfg.nslots == 1 and cfg.prep_width == wp, (cfg.nslots, cfg.prep_width)
    return LineaAIR([cfg])


def keyed_sum_rows(wp, h, x0=5):
    """(fixed rows h x wp, main rows h x 1, the public values after [alpha,
    delta]) of a trace that satisfies keyed_sum(wp); the fixed cells differ in
    every row and column and reach the top limb"""
    fixed = [[(R - 1 - 7 * j * j - 3 - 11 * i * (i + 1)) % R if (i + j) % 3 == 0 else (7 * j * j + 3 + 11 * i) % R
              for i in range(wp)] for j in range(h)]
    main, x = [], x0
    for j in range(h):
        main.append([x])
        x = (x * x + sum(fixed[j])) % R
    return fixed, main, [x0]


def joined(fixed, main):
    """layout a's trace rows: the fixed columns first"""
    return [list(f) + list(m) for f, m in zip(fixed, main)]


# ------------------------------------------------------- reference prover
# An independent big-integer prover for the protocol of include/lsp.h
# (lsp_verify_preprocessed), assembled from oracle.pyoracle's pieces.  With
# fixed = None it is plain uni-stark over a program AIR and writes LSPPRF02.
import struct  # noqa: E402

from oracle import pyoracle as O  # noqa: E402


def log_quotient_degree(air, pd=1):
    d = max(2, max(x for c in air.configs for x in program_degrees(c, pd)))
    return (d - 2).bit_length()  # ceil(log2(d - 1))


def quotient_values(air, lde, plde, log_h, log_q, alpha, pub):
    logQ = log_h + log_q
    Q = 1 << logQ
    view = [lde[O.bitrev(k, logQ)] for k in range(Q)]
    pview = [plde[O.bitrev(k, logQ)] for k in range(Q)] if plde is not None else [None] * Q
    first, last, trans, inv_z = O.selectors_on_coset(log_h, logQ)
    step = 1 << log_q
    out = []
    for i in range(Q):
        n = (i + step) % Q
        acc = 0
        for c in eval_air(air, view[i], view[n], pub, first[i], last[i], trans[i], pview[i], pview[n]):
            acc = (acc * alpha + c) % R
        out.append(acc * inv_z[i] % R)
    return out


def preprocess(fixed, pp, log_blowup=3):
    """(the LDE, its Merkle tree) of the fixed matrix: what lsp_preprocess commits"""
    plde = O.coset_lde_batch(fixed, log_blowup, O.GENERATOR)
    return plde, O.merkle_commit([plde], pp)


def prove(air, main, fixed, pub, pp, fri=None, public_degree=1):
    """-> (proof bytes, log): LSPPRF03 with a fixed matrix, LSPPRF02 without"""
    fri = fri or O.FriParams()
    h, w = len(main), len(main[0])
    wp = len(fixed[0]) if fixed is not None else 0
    log_h, lb = O.log2_strict(h), fri.log_blowup
    log_q = log_quotient_degree(air, public_degree)
    q = 1 << log_q
    assert log_q <= lb
    lde = O.coset_lde_batch(main, lb, O.GENERATOR)
    t_tree = O.merkle_commit([lde], pp)
    plde, p_tree = preprocess(fixed, pp, lb) if wp else (None, None)
    ch = O.HashChallenger(pp, mont_bits=fri.sample_bits_montgomery)
    if fri.observe_log_degree:
        ch.observe(log_h)
    ch.observe(t_tree.root)
    if wp:
        ch.observe(p_tree.root)  # U13
    if fri.observe_public_values:
        ch.observe_slice(pub)
    alpha = ch.sample()
    qv = quotient_values(air, lde, plde, log_h, log_q, alpha, pub)
    gq = O.two_adic_generator(log_h + log_q)
    chunk_rows = [qv[k * q:(k + 1) * q] for k in range(h)]
    shifts = [O.inv(pow(gq, j, R)) for j in range(q)]
    q_lde = O.coset_lde_batch(chunk_rows, lb, shifts)
    q_tree = O.merkle_commit([[[r[j]] for r in q_lde] for j in range(q)], pp)
    ch.observe(q_tree.root)
    zeta = ch.sample()
    zeta_next = zeta * O.two_adic_generator(log_h) % R
    N, logN = h << lb, log_h + lb
    invd = dict(zip((zeta, zeta_next), O.inverse_denominators(logN, O.GENERATOR, [zeta, zeta_next])))
    tl = O.interpolate_coset(lde[:h], O.GENERATOR, zeta)
    tn = O.interpolate_coset(lde[:h], O.GENERATOR, zeta_next)
    qc = O.interpolate_coset(q_lde[:h], O.GENERATOR, zeta)
    pl = O.interpolate_coset(plde[:h], O.GENERATOR, zeta) if wp else []
    pn = O.interpolate_coset(plde[:h], O.GENERATOR, zeta_next) if wp else []
    if fri.observe_opened_values:
        ch.observe_slice(tl + tn + qc + pl + pn)
    alpha_fri = ch.sample()
    ro = [0] * N
    off = O.open_reduce(lde, [invd[zeta], invd[zeta_next]], [tl, tn], alpha_fri, 1, ro)
    for j in range(q):
        off = O.open_reduce([[r[j]] for r in q_lde], [invd[zeta]], [[qc[j]]], alpha_fri, off, ro)
    if wp:
        off = O.open_reduce(plde, [invd[zeta], invd[zeta_next]], [pl, pn], alpha_fri, off, ro)
    folded, trees = ro, []
    while len(folded) > 1 << (lb + fri.log_final_poly_len):
        tr = O.merkle_commit([[[folded[2 * i], folded[2 * i + 1]] for i in range(len(folded) // 2)]], pp)
        ch.observe(tr.root)
        trees.append(tr)
        folded = O.fold_vector(folded, ch.sample())
    coeffs = O.idft(O.reverse_slice_index_bits(folded))
    assert fri.log_final_poly_len == 0 and all(c == 0 for c in coeffs[1:]), "final poly degree too high"
    if fri.observe_final_poly:
        ch.observe(coeffs[0])
    pow_w = ch.grind(fri.proof_of_work_bits)
    fe = O.to_canon_bytes
    out = bytearray(b"LSPPRF03" if wp else b"LSPPRF02")
    out += struct.pack("<6I", log_h, log_q, w, fri.num_queries, len(trees), 1)
    if wp:
        out += struct.pack("<I", wp)
    for v in [t_tree.root, q_tree.root] + tl + tn + qc + pl + pn + [t.root for t in trees] + [coeffs[0], pow_w]:
        out += fe(v)
    marks = {"prep_local": 8 + 28 + 32 * (2 + 2 * w + q), "prep_next": 8 + 28 + 32 * (2 + 2 * w + q + wp)}

    def opening(row, path):
        b = b"".join(fe(v) for v in row) + struct.pack("<I", len(path))
        return b + b"".join(fe(v) for v in path)

    for k in range(fri.num_queries):
        idx = ch.sample_bits(logN)
        rows, path = O.merkle_open(t_tree, idx)
        out += opening(rows[0], path)
        rows, path = O.merkle_open(q_tree, idx)
        out += opening([x[0] for x in rows], path)
        if wp:
            rows, path = O.merkle_open(p_tree, idx)
            if k == 0:
                marks["prep_row"] = len(out)
                marks["prep_path"] = len(out) + 32 * wp + 4
            out += opening(rows[0], path)
        for r_, tr in enumerate(trees):
            ii = idx >> r_
            rows, path = O.merkle_open(tr, ii >> 1)
            out += opening([rows[0][(ii ^ 1) & 1]], path)
    log = dict(marks=marks, prep_root=p_tree.root if wp else None, zeta=zeta, alpha=alpha, prep_local=pl,
               prep_next=pn, log_q=log_q)
    return bytes(out), log


def parse(b):
    """the reference's own reading of LSPPRF02 / LSPPRF03 bytes: a dict of ints
    (elements canonical), queries as dicts; consumes the bytes exactly"""
    prep = b[:8] == b"LSPPRF03"
    assert prep or b[:8] == b"LSPPRF02"
    off = 8

    def u32():
        nonlocal off
        off += 4
        return struct.unpack_from("<I", b, off - 4)[0]

    def fes(n):
        nonlocal off
        out = [int.from_bytes(b[off + 32 * i:off + 32 * i + 32], "little") for i in range(n)]
        off += 32 * n
        return out

    log_h, log_q, w, nq, nr, nf = (u32() for _ in range(6))
    wp = u32() if prep else 0
    q = 1 << log_q
    p = dict(log_h=log_h, log_q=log_q, w=w, wp=wp, trace_root=fes(1)[0], quotient_root=fes(1)[0], trace_local=fes(w),
             trace_next=fes(w), chunks=fes(q), prep_local=fes(wp), prep_next=fes(wp), fri_roots=fes(nr),
             final_poly=fes(nf), pow_witness=fes(1)[0], queries=[])
    for _ in range(nq):
        qq = dict(trow=fes(w), tpath=fes(u32()), qrow=fes(q), qpath=fes(u32()))
        if prep:
            qq.update(prow=fes(wp), ppath=fes(u32()))
        qq["steps"] = [(fes(1)[0], fes(u32())) for _ in range(nr)]
        p["queries"].append(qq)
    assert off == len(b)
    return p
