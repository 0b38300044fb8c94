"""Inputs and expectations for the witness kernels' edges, shared by
tests/test_witness_cases.py (the cases are what they claim, against pyoracle)
and tests/test_gpu_witness_edges.py (the device computes them).

Three kinds of thing live here, none of which touches a GPU:

* closed forms for two telescoping inputs -- a permutation whose B is A
  rotated by one row, a lookup whose A is its table rotated by one row --
  so that a scan of millions of rows can be checked at any row without
  scanning on the host;
* models of two device functions written from csrc/k_witness.hip: the
  occurrence table's key_hash (to build keys that collide in it) and the
  seeded generator k_gen_raw_perm / gen_value;
* the named lookup and permutation cases of the occurrence-table, filter and
  column-count tests, as canonical integers.

Values are canonical integers in [0, P).  Where a test needs particular
Montgomery words (the hash reads words 0 and 2 of the stored element), the
integer is the one whose Montgomery form is those words: to_words() gives
them back.
"""
import functools

from oracle import pyoracle as O

P = O.P
M64 = (1 << 64) - 1
SC_TILE = 2048  # the scan's tile (SC_THREADS * SC_PER in k_witness.hip)


@functools.lru_cache(maxsize=None)
def challenges():
    s = O.setup_from_seed()
    return s.alpha, s.delta


# ------------------------------------------------------------ integer helpers
def to_words(v):
    """the four 64-bit little-endian words of v's Montgomery form"""
    m = v % P * O.MONT_R % P
    return tuple((m >> (64 * k)) & M64 for k in range(4))


def from_words(w):
    """the canonical integer whose Montgomery form is the words w (w < P as an integer)"""
    m = sum(int(x) << (64 * k) for k, x in enumerate(w))
    assert m < P, "not a canonical element"
    return m * O.MONT_R_INV % P


def batch_inv(xs):
    """the inverses of non-zero xs mod P with one exponentiation"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % P
    assert acc, "zero among the values to invert"
    inv = pow(acc, P - 2, P)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % P
        inv = inv * xs[i] % P
    return out


def rand_fr(seed, n):
    rng = O.SplitMix64(seed)
    return [rng.sample_fr() for _ in range(n)]


def shuffled(seed, items):
    """a Fisher-Yates shuffle of items, deterministic in the seed"""
    rng = O.SplitMix64(seed)
    out = list(items)
    for i in range(len(out) - 1, 0, -1):
        j = rng.below(i + 1)
        out[i], out[j] = out[j], out[i]
    return out


# --------------------------------------------------------------- closed forms
def rotation_perm_rows(val, n, rows):
    """Permutation, one column each side, b[i] = a[(i - 1) mod n]: the trace
    rows [a, b, b_inverse, check] at `rows`.  val(i) is the integer a[i].

    check[i] = prod_{j <= i} (a[j] + d) / (a[j-1] + d) telescopes to
    (a[i] + d) / (a[n-1] + d); b_inverse[i] = 1 / (a[i-1] + d)."""
    _, d = challenges()
    rows = list(rows)
    inv = batch_inv([(val((i - 1) % n) + d) % P for i in rows] + [(val(n - 1) + d) % P])
    last = inv.pop()
    return [[val(i), val((i - 1) % n), bi, (val(i) + d) * last % P] for i, bi in zip(rows, inv)]


def rotation_lookup_rows(val, n, rows):
    """Lookup, one table of one column with distinct values b, a[i] =
    b[(i - 1) mod n], every filter 1: the trace rows [a, b, a_filter, b_filter,
    a_inverse, b_inverse, multiplicity, sum] at `rows`.  val(i) is the integer b[i].

    Every key is looked up once, so every multiplicity is 1 and
    sum[i] = sum_{j <= i} 1 / (b[j-1] + d) - 1 / (b[j] + d) telescopes to
    1 / (b[n-1] + d) - 1 / (b[i] + d)."""
    _, d = challenges()
    rows = list(rows)
    k = len(rows)
    inv = batch_inv([(val((i - 1) % n) + d) % P for i in rows] + [(val(i) + d) % P for i in rows] +
                    [(val(n - 1) + d) % P])
    last = inv.pop()
    return [[val((i - 1) % n), val(i), 1, 1, inv[j], inv[k + j], 1, (last - inv[k + j]) % P]
            for j, i in enumerate(rows)]


def rotation_perm_input(n, seed=None):
    """(a, b) of the rotation permutation with random a"""
    a = rand_fr(0x5043 + n if seed is None else seed, n)
    return [a], [a[-1:] + a[:-1]]


def rotation_lookup_input(n, seed=None):
    """(a, b, a_filter, b_filter) of the rotation lookup with distinct random b"""
    b = rand_fr(0x4C55 + n if seed is None else seed, n)
    assert len(set(b)) == n
    return [b[-1:] + b[:-1]], [[b]], [1] * n, [[1] * n]


PERM_SCAN_SIZES = (1, 2, 7, 8, 9, 255, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 5)
LOOKUP_SCAN_SIZES = (1, 7, 2047, 2049, 4097)
# two levels of tile aggregates: 2049 tiles with a last tile of one element
# (and a second level of two tiles, the last of one aggregate); 2050 tiles
# with a last tile of one element after a full one
PERM_BIG_SIZES = (2048 * 2048 + 1, (1 << 22) + 2049)
LOOKUP_BIG_SIZE = (1 << 22) + 1


def big_rows(n, seed=0x524F5753, random_rows=2000):
    """the rows of a big scan that must be compared: both ends, the rows around
    the tile boundaries k 2048 for the first tiles, the tiles around the second
    level's boundary (tile 2048) and the last tile, and seeded random rows"""
    tiles = (n + SC_TILE - 1) // SC_TILE
    rows = set(range(min(16, n))) | set(range(max(0, n - 16), n))
    for k in (1, 2, 2047, 2048, 2049, tiles - 1):
        rows |= {k * SC_TILE - 1, k * SC_TILE, k * SC_TILE + 7}
    rng = O.SplitMix64(seed)
    extra = set()
    while len(extra) < random_rows:
        extra.add(rng.below(n))
    return sorted(r for r in rows | extra if 0 <= r < n)


# ------------------------------------------------- the occurrence table's hash
def key_hash(w):
    """key_hash of csrc/k_witness.hip on the four 64-bit Montgomery words of a
    key: words 0 and 2 only.  This MIRRORS the kernel's formula and must be
    revisited when that function changes -- a model that has drifted makes no
    test fail, it only turns the colliding keys below into ordinary ones."""
    x = (w[0] ^ (w[2] * 0x9E3779B97F4A7C15)) & M64
    x ^= x >> 29
    x = (x * 0xBF58476D1CE4E5B9) & M64
    return (x ^ (x >> 32)) & 0xFFFFFFFF


def occ_capacity(m):
    """the table's slots for m records (occ_capacity in k_witness.hip)"""
    c = 64
    while c < 2 * m:
        c <<= 1
    return c


@functools.lru_cache(maxsize=None)
def colliding_keys(count, cap, slot):
    """`count` Montgomery word quadruples with the same words 0 and 2 -- one
    hash -- and key_hash & (cap - 1) == slot.  Words 1 and 3 differ from key to
    key; word 3 is below 2^58, so every quadruple is a canonical element, and
    all are distinct."""
    assert cap & (cap - 1) == 0 and 0 <= slot < cap
    w2 = 0x0123456789ABCDEF
    w0 = 1
    while key_hash((w0, 0, w2, 0)) & (cap - 1) != slot:
        w0 += 1
    rng = O.SplitMix64((cap << 20) ^ slot)
    keys, seen = [], set()
    while len(keys) < count:
        w1, w3 = rng.next_u64(), rng.next_u64() & ((1 << 58) - 1)
        if w1 not in seen:
            seen.add(w1)
            keys.append((w0, w1, w2, w3))
    return tuple(keys)


# ------------------------------------------------------- the device generator
def _smix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def gen_value(seed, c, i):
    """gen_value of k_witness.hip: four mixed words of a counter made of
    (seed, column, row), the top word cut to 60 bits (252 bits in all, below P).
    The kernel stores this integer's Montgomery form: it is the field element."""
    base = (seed * 0x9E3779B97F4A7C15 + (c << 40) + (i << 2)) & M64
    v = 0
    for k in range(4):
        v |= _smix((base + k + 0x632BE59BD9B4E019) & M64) << (64 * k)
    return v & ((1 << 252) - 1)


def gen_row_map(seed, log_n):
    """(mul, add) of lsp_gen_permutation_trace_device (witness.cpp): B's row i is
    A's row (mul i + add) mod 2^log_n, mul odd"""
    mul = (((seed * 0xD1B54A32D192ED03) & M64) ^ 0x5851F42D4C957F2D) | 1
    add = (seed * 0xA24BAED4963EE407 + 0x9FB21C651E98DF25) & M64
    return mul, add


def gen_raw_perm(seed, log_n, ncols):
    """(a, b) of k_gen_raw_perm: a[c][i] = gen_value(seed, c, i), b[c][i] =
    a[c][(mul i + add) mod n], the same row map for every column"""
    n = 1 << log_n
    mul, add = gen_row_map(seed, log_n)
    a = [[gen_value(seed, c, i) for i in range(n)] for c in range(ncols)]
    src = [((mul * i + add) & M64) & (n - 1) for i in range(n)]
    return a, [[col[j] for j in src] for col in a]


GEN_SHAPES = ((1, 1), (5, 3), (11, 3), (13, 2))
GEN_SEEDS = (1, 0xD1CEB01DFACEF00D)  # the bench's seed; one whose products wrap 2^64


@functools.lru_cache(maxsize=None)
def gen_trace_columns(seed, log_n, ncols):
    """the generator's trace: O.perm_witness of the model's columns"""
    a, b = gen_raw_perm(seed, log_n, ncols)
    return O.perm_witness(a, b, *challenges())[1]


# -------------------------------------------------------------- lookup cases
# filter values that are not zero but whose Montgomery form has zero low words,
# beside 2 and r - 1
HIGH_FILTERS = (from_words((0, 0, 0, 0x0123456789ABCDE)), from_words((0, 0, 0xFEDCBA9876543210, 0)), 2, P - 1)


def _lookup_wrap8():
    """8 keys of one hash at slot 61 of a 64-slot table (n = 8: 16 records):
    the chain runs 61, 62, 63, 0, 1, ...; a[i] = keys[3 i mod 8]"""
    keys = [from_words(w) for w in colliding_keys(8, 64, 61)]
    return [[keys[3 * i % 8] for i in range(8)]], [[keys]], [1] * 8, [[1] * 8]


CHAIN_N, CHAIN_KEYS, CHAIN_SLOT = 512, 300, 2048 - 100


def _lookup_chain300():
    """n = 512 (1024 records, 2048 slots): 300 keys of one hash whose chain
    starts 100 slots before the table's end, among 212 ordinary table values.
    A holds 75 of the keys three times each, the other 225 once, and 62
    ordinary values, in shuffled order -- many waves extend and walk one chain"""
    keys = [from_words(w) for w in colliding_keys(CHAIN_KEYS, occ_capacity(2 * CHAIN_N), CHAIN_SLOT)]
    plain = rand_fr(0x434841, CHAIN_N - CHAIN_KEYS)
    b = shuffled(1, keys + plain)
    a = shuffled(2, keys[:75] * 3 + keys[75:] + plain[:CHAIN_N - 450])
    assert len(a) == CHAIN_N and len(set(b)) == CHAIN_N
    return [a], [[b]], [1] * CHAIN_N, [[1] * CHAIN_N]


def _lookup_both_tables():
    """two tables.  K1 sits in both tables on row 3: table 0 comes first.  K2
    sits on row 2 of table 1 and on row 5 of table 0 only: the earlier row
    takes the count, although table 0's records come first in the key array"""
    n = 8
    k1, k2 = 1001, 1002
    b0 = [10 + i for i in range(n)]
    b1 = [30 + i for i in range(n)]
    b0[3] = b1[3] = k1
    b1[2] = b0[5] = k2
    a = [k1, k2, k2, 10, k1, k2, 31, 37]
    return [a], [[b0], [b1]], [1] * n, [[1] * n, [1] * n]


def _lookup_first_disabled():
    """K's first table entry (row 2) is disabled, its second (row 5) enabled:
    the second takes the count of the three enabled A rows; a fourth A row
    holding K is disabled and is not counted"""
    n = 8
    k = 1001
    b = [10 + i for i in range(n)]
    b[2] = b[5] = k
    bf = [1] * n
    bf[2] = 0
    a = [k, 10, k, 11, k, 13, k, 14]
    af = [1] * n
    af[6] = 0
    return [a], [[b]], af, [bf]


def _lookup_only_disabled():
    """an enabled A row whose key only disabled table entries hold: the sum does not close"""
    a, b, af, bf = _lookup_first_disabled()
    bf[0][5] = 0
    return a, b, af, bf


ONE_KEY_N = 4097


def _lookup_one_key():
    """every one of 4097 A rows holds K; the table holds K on rows 2500 and
    3000: row 2500 gets the count 4097, every other multiplicity is 0"""
    n = ONE_KEY_N
    k = 123456789
    b = list(range(1, n + 1))
    b[2500] = b[3000] = k
    return [[k] * n], [[b]], [1] * n, [[1] * n]


def _lookup_high_filters():
    """filters drawn from HIGH_FILTERS and 0, for A and for the table: every
    non-zero one enables its row, whichever words of it are non-zero"""
    n = 10
    f = HIGH_FILTERS
    b = [100 + i for i in range(n)]
    bf = [f[0], f[1], f[2], f[3], 0, f[0], f[1], 0, f[3], f[2]]
    #    looked up by A:  0     1     2     3   -   5     -   -   8     -
    a = [100, 101, 102, 103, 104, 105, 100, 108, 107, 100]
    af = [f[0], f[1], f[2], f[3], 0, f[1], f[0], f[3], 0, f[2]]
    return [a], [[b]], af, [bf]


def _lookup_na2():
    """A of two columns against a table of one: a0 alpha + a1 = b[j]"""
    al, _ = challenges()
    n = 9
    b = rand_fr(0x4E4132, n)
    a0 = rand_fr(0x4E4133, n)
    pick = [(5 * i + 2) % n if i % 3 else 4 for i in range(n)]
    a1 = [(b[j] - x * al) % P for x, j in zip(a0, pick)]
    bf = [1] * n
    af = [1] * n
    af[7] = 0
    return [a0, a1], [[b]], af, [bf]


def _lookup_nbc2():
    """A of one column against two tables of two columns: a = b0 alpha + b1 of some entry"""
    al, _ = challenges()
    n = 9
    tabs = [[rand_fr(0x4E4240 + 2 * t + c, n) for c in range(2)] for t in range(2)]
    a = [(tabs[i % 2][0][(4 * i + 1) % n] * al + tabs[i % 2][1][(4 * i + 1) % n]) % P for i in range(n)]
    bf = [[1] * n, [1] * n]
    bf[1][0] = 0  # no A row looks (table 1, row 0) up: 4 i + 1 = 0 mod 9 at i = 2, an even i
    return [a], tabs, [1] * n, bf


LOOKUP_CASES = {
    "wrap8": _lookup_wrap8,
    "chain300": _lookup_chain300,
    "both_tables": _lookup_both_tables,
    "first_disabled": _lookup_first_disabled,
    "only_disabled": _lookup_only_disabled,
    "one_key": _lookup_one_key,
    "high_filters": _lookup_high_filters,
    "na2_nbc1": _lookup_na2,
    "na1_nbc2": _lookup_nbc2,
}
LOOKUP_FAILING = ("only_disabled",)
LOOKUP_TABLE_CASES = ("wrap8", "chain300", "both_tables", "first_disabled", "one_key", "high_filters")
LOOKUP_UNEVEN = ("na2_nbc1", "na1_nbc2")


# --------------------------------------------------------- permutation cases
def _perm_na2_nb1():
    """b0 is a shuffle of a0 alpha + a1"""
    al, _ = challenges()
    n = 11
    a0, a1 = rand_fr(0x504132, n), rand_fr(0x504133, n)
    return [a0, a1], [shuffled(3, [(x * al + y) % P for x, y in zip(a0, a1)])]


def _perm_na1_nb3():
    """a0 is a shuffle of b0 alpha^2 + b1 alpha + b2"""
    al, _ = challenges()
    n = 11
    b = [rand_fr(0x504233 + c, n) for c in range(3)]
    return [shuffled(4, [((x * al + y) * al + z) % P for x, y, z in zip(*b)])], b


PERM_CASES = {"na2_nb1": _perm_na2_nb1, "na1_nb3": _perm_na1_nb3}


@functools.lru_cache(maxsize=None)
def lookup_columns(name):
    """the reference's columns of a lookup case (computed once; do not modify)"""
    return O.lookup_witness(*LOOKUP_CASES[name](), *challenges())[1]


@functools.lru_cache(maxsize=None)
def perm_columns(name):
    return O.perm_witness(*PERM_CASES[name](), *challenges())[1]


# The uneven cases as lsp_raw_trace_push sees them at a height above their
# longest column: every raw column, the filters too, resized with zero words
# (RawTrace's Vec::resize).  A padded row adds delta / delta to the product
# and, its filters being 0, nothing to the sum.
PAD_ROWS = 3


def _padded(cols, h):
    return [list(c) + [0] * (h - len(c)) for c in cols]


def padded_perm_case(name):
    a, b = PERM_CASES[name]()
    h = max(len(c) for c in a + b) + PAD_ROWS
    return _padded(a, h), _padded(b, h)


def padded_lookup_case(name):
    a, b, af, bf = LOOKUP_CASES[name]()
    h = max(len(c) for c in a + [c for t in b for c in t]) + PAD_ROWS
    return _padded(a, h), [_padded(t, h) for t in b], _padded([af], h)[0], _padded(bf, h)


@functools.lru_cache(maxsize=None)
def padded_perm_columns(name):
    return O.perm_witness(*padded_perm_case(name), *challenges())[1]


@functools.lru_cache(maxsize=None)
def padded_lookup_columns(name):
    return O.lookup_witness(*padded_lookup_case(name), *challenges())[1]


@functools.lru_cache(maxsize=None)
def rotation_perm_columns(n):
    return O.perm_witness(*rotation_perm_input(n), *challenges())[1]


@functools.lru_cache(maxsize=None)
def rotation_lookup_columns(n):
    return O.lookup_witness(*rotation_lookup_input(n), *challenges())[1]
