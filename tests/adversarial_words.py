"""Adversarial Montgomery *words* and matrix fillings made of them, shared by
tests/test_adversarial_words.py (CPU) and tests/test_gpu_adversarial_words.py.

A word is the 256-bit integer W that lies in memory; its value is
W * 2^-256 mod r.  The parity suites draw uniform *values* and convert them, so
every word they feed the kernels is pseudo-random.  What can go wrong in the
device code depends on the word: a 29-bit limb of all ones, a top limb equal to
the modulus's own, a word sum that lands exactly on r, a lazily reduced
limb-wise sum at the top of its range.  The corpus below is built from such
words directly; reference values come from them through `from_mont`.

CORPUS = base words, then for every base word W the ark word W * 2^-5 mod r
(the word whose device-internal 29-bit form x * 2^261 mod r is W), then for
every word so far its additive partners r - W, r - W - 1 and r - W + 1 where
canonical.  Deduplicated, order fixed.  No tests in this module.
"""
import numpy as np

from linea_stark_prover_amd.field import MODULUS, from_mont

R = MODULUS
M29 = (1 << 29) - 1
M32 = (1 << 32) - 1
W_SAT = ((R >> 232) << 232) - 1  # low 29-bit limbs all 0x1fffffff, top limb r's minus one


def _alt(lo, top):
    return sum(lo << (29 * i) for i in range(8)) | (top << 232)


BASE = (
    [0, 1, 2, R - 1, R - 2,
     (1 << 252) - 1, 1 << 252,
     W_SAT, (R >> 232) << 232,
     (1 << 232) - 1, 1 << 232,
     ((R >> 224) << 224) - 1]                      # the 32-bit-limb analogue of W_SAT (8 x 32 FIPS product)
    + [M29 << (29 * i) for i in range(8)]          # one saturated 29-bit limb
    + [M32 << (32 * i) for i in range(7)]          # one saturated 32-bit limb
    + [_alt(0x0AAAAAAA, 0x0AAAAA), _alt(0x15555555, 0x055555)]
    + [pow(2, e, R) for e in (256, 512, 261, 266)]
    + [(R - 1) // 2, (R + 1) // 2]
)


def _dedup(ws):
    seen, out = set(), []
    for w in ws:
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


BASE = _dedup(BASE)
INV32 = pow(32, -1, R)
PREIMAGES = [w * INV32 % R for w in BASE]           # PREIMAGES[i] * 2^5 = BASE[i] (mod r)
_core = _dedup(BASE + PREIMAGES)
_partners = [p for w in _core for p in (R - w, R - w - 1, R - w + 1) if 0 <= p < R]
CORPUS = _dedup(_core + _partners)
N = len(CORPUS)
NONZERO = [w for w in CORPUS if w]


# points z and coset shifts for the open-phase tests: fixed, chosen so that no
# z lies on a coset shift * H_N (z^N != shift^N) for any N up to 2^11
Z_WORDS = [W_SAT, R - 1, W_SAT * INV32 % R]
SHIFT_WORDS = [(R >> 232) << 232, (R - 1) * INV32 % R, 2]


def weight(w):
    """set bits of the word: the `heaviest` words have the most"""
    return bin(w).count("1")


def heaviest(k):
    """the k words with the most set bits, ties in corpus order"""
    return sorted(CORPUS, key=lambda w: -weight(w))[:k]


def arr(words, shape=None):
    """words -> uint64 limb array (..., 4), straight from the words (no conversion)"""
    ws = [int(w) for w in words]
    a = np.frombuffer(b"".join(w.to_bytes(32, "little") for w in ws), dtype=np.uint64).reshape(-1, 4).copy()
    return a if shape is None else a.reshape(tuple(shape) + (4,))


def words_of(a):
    """uint64 limb array -> list of words"""
    raw = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


_RINV = pow(1 << 256, -1, R)


def value(w):
    """the field element a word stands for"""
    return w * _RINV % R


def values(a):
    """uint64 limb array -> canonical values (field.from_mont)"""
    return from_mont(a)


# ------------------------------------------------------------------ fillings
# each returns an h x w list of rows of words
def const(h, w, W):
    return [[W] * w for _ in range(h)]


def by_column(h, w):
    return [[CORPUS[c % N] for c in range(w)] for _ in range(h)]


def cyclic(h, w):
    return [[CORPUS[(7 * i + c) % N] for c in range(w)] for i in range(h)]


def alternate(h, w, W):
    return [[W if i % 2 == 0 else 0] * w for i in range(h)]


def spike(h, w, W, at=None):
    """one cell W (by default the last row, middle column), the rest 0"""
    r, c = (h - 1, w // 2) if at is None else at
    m = [[0] * w for _ in range(h)]
    m[r][c] = W
    return m


def fillings(h, w, W=W_SAT):
    """name -> h x w rows of words, every filling (the parametrised ones with W)"""
    return {"const": const(h, w, W), "by_column": by_column(h, w), "cyclic": cyclic(h, w),
            "alternate": alternate(h, w, W), "spike": spike(h, w, W)}


FILLINGS = ("const", "by_column", "cyclic", "alternate", "spike")


def mat(rows):
    """h x w rows of words -> (h, w, 4) uint64"""
    h, w = len(rows), len(rows[0])
    return arr([x for r in rows for x in r], (h, w))


# the same fillings as (h, w) arrays of corpus indices, for the large shapes:
# CORPUS_ARR[index matrix] is the limb array, VALUES[i] the value of CORPUS[i]
CORPUS_ARR = arr(CORPUS)
VALUES = [value(w) for w in CORPUS]
INDEX = {w: i for i, w in enumerate(CORPUS)}


def fill_index(name, h, w, W=W_SAT):
    """filling `name` of an h x w matrix as corpus indices (CORPUS[0] is 0)"""
    k = INDEX[W]
    i, c = np.arange(h).reshape(h, 1), np.arange(w).reshape(1, w)
    if name == "const":
        return np.full((h, w), k)
    if name == "by_column":
        return np.broadcast_to(c % N, (h, w)).copy()
    if name == "cyclic":
        return (7 * i + c) % N
    if name == "alternate":
        return np.broadcast_to(np.where(i % 2 == 0, k, 0), (h, w)).copy()
    assert name == "spike"
    m = np.zeros((h, w), dtype=np.int64)
    m[h - 1, w // 2] = k
    return m


def index_mat(idx):
    """corpus index matrix -> (h, w, 4) uint64"""
    return np.ascontiguousarray(CORPUS_ARR[idx])


def index_values(idx):
    """corpus index matrix -> h rows of w values"""
    return [[VALUES[j] for j in row] for row in idx.tolist()]
