"""The reference's E-step of one sentence re-stated in numpy over a ``latticeref.Lattice``: what ExpectedCounts (kernels_nbest.h
mode 6) is compared with.  TEST INFRASTRUCTURE ONLY.

``Lattice::PopulateMarginal`` (src/unigram_model.cc:235-261) in the reference's order and float32 arithmetic, as
tests/latticescore.py restates the entropy:

    ForwardAlgorithm(1.0) (:200-216)    A[pos] = LogSumExp over the edges into pos, by ascending begin, of score + A[begin]
    BackwardAlgorithm(1.0) (:218-233)   B[pos] = LogSumExp over the edges from pos, in INSERTION order -- the trie's matches by
                                        increasing length, the unknown edge last -- of score + B[end];  B[len] = 0
    marginal (:248-257)                 t = ((A[begin] + score) + B[end]) - Z, every sum rounded to float32; p = exp(double(t))
    contribution                        q = llrint(freq * p * 2^24), to nearest even, into a 64-bit accumulator per id

LogSumExp's double ``exp`` / ``log`` and the marginal's ``exp`` are glibc's, through ctypes: numpy's are not.  ``lse_float`` is
the all-float32 variant (``expf`` / ``logf``) the device bound of tests/test_expected_counts.py is measured with.  The golden
cases of tests/golden/expected_counts.npz are defined here too, for scripts/make_estep_golden.py and the tests."""
import ctypes
import ctypes.util
import functools
import os

import numpy as np

from tests import latticescore as ls

F = np.float32
FRAC_BITS = 24
ONE = float(1 << FRAC_BITS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expected_counts.npz")
# every sentence of tests/golden/lattice_scores.json at freq 1; the 64- and 300-byte ones at these weights too (exact in float)
EXTRA_FREQS = (3, 1 << 20)
EXTRA_LENGTHS = (64, 300)


def _libm():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for name in ("exp", "log"):
        fn = getattr(m, name)
        fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double]
    for name in ("expf", "logf"):
        fn = getattr(m, name)
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return m


_M = _libm()


def lse_double(x, y):
    """LogSumExp (:47-59) as the reference's build has it: double exp and log, the result rounded to float32."""
    vmin, vmax = (x, y) if x < y else (y, x)
    if vmax > F(vmin + F(50.0)):
        return vmax
    return F(float(vmax) + _M.log(_M.exp(float(F(vmin - vmax))) + 1.0))


def lse_float(x, y):
    """The same with an all-float32 libm: a larger perturbation than a device's double exp / log rounded to float."""
    vmin, vmax = (x, y) if x < y else (y, x)
    if vmax > F(vmin + F(50.0)):
        return vmax
    return F(vmax + F(_M.logf(F(F(_M.expf(F(vmin - vmax))) + F(1.0)))))


def from_order(lat):
    """Per position the edges beginning there in the reference's insertion order: by length, the unknown edge last."""
    unk = lat.model.unk_id
    return [sorted((int(e) for e in lat._from[p]), key=lambda e: (int(lat.id[e]) == unk, int(lat.ce[e]))) for p in range(lat.n_chars + 1)]


def forward32(lat, lse=lse_double):
    sc = lat.score.astype(F)
    A = np.zeros(lat.n_chars + 1, dtype=F)
    for p in range(1, lat.n_chars + 1):
        acc = None
        for e in lat._into[p]:
            v = F(sc[e] + A[lat.cb[e]])
            acc = v if acc is None else lse(acc, v)
        A[p] = acc
    return A


def backward32(lat, lse=lse_double):
    """B float32[n_chars + 1]: the reference's beta of a node ENDING at a position."""
    sc = lat.score.astype(F)
    order = from_order(lat)
    B = np.zeros(lat.n_chars + 1, dtype=F)
    for p in range(lat.n_chars - 1, -1, -1):
        acc = None
        for e in order[p]:
            v = F(sc[e] + B[lat.ce[e]])
            acc = v if acc is None else lse(acc, v)
        B[p] = acc
    return B


def viterbi_nodes32(lat):
    """Nodes on Lattice::Viterbi()'s path (:161-198): float32 scores, the first best left node wins."""
    if lat.n_chars == 0:
        return 0
    sc = lat.score.astype(F)
    bt = np.zeros(len(lat), dtype=F)
    prev = np.full(len(lat), -1, dtype=np.int64)
    for e in range(len(lat)):                                     # edges are sorted by begin
        into = lat._into[int(lat.cb[e])]
        if len(into) == 0:
            bt[e] = F(F(0.0) + sc[e])
            continue
        v = (bt[into] + sc[e]).astype(F)
        k = int(np.argmax(v))                                     # the first of equal ones
        bt[e], prev[e] = v[k], into[k]
    into = lat._into[lat.n_chars]
    e = int(into[int(np.argmax(bt[into]))])                       # EOS: score 0
    count = 0
    while e >= 0:
        count += 1
        e = int(prev[e])
    return count


def marginal_q(lat, freq=1, lse=lse_double):
    """-> (q int64 per edge, {id: accumulator}, Z float32): the integer contributions of one sentence at weight ``freq``."""
    if lat.n_chars == 0:
        return np.zeros(0, dtype=np.int64), {}, F(0.0)
    sc = lat.score.astype(F)
    A, B = forward32(lat, lse), backward32(lat, lse)
    Z = A[lat.n_chars]
    t = (((A[lat.cb] + sc).astype(F) + B[lat.ce]).astype(F) - Z).astype(F)
    p = np.array([_M.exp(float(x)) for x in t], dtype=np.float64)
    q = np.rint(float(freq) * p * ONE).astype(np.int64)           # to nearest, ties to even
    acc = {}
    for i, v in zip(lat.id.tolist(), q.tolist()):
        if v:
            acc[i] = acc.get(i, 0) + v
    return q, acc, Z


def ulp32(x):
    return float(np.spacing(F(abs(float(x)))))


def cases():
    """[(sentence index into lattice_scores.json's sentences, freq)] in the golden file's order."""
    out = []
    for i, s in enumerate(ls.golden()["sentences"]):
        out.append((i, 1))
        if s["name"].lstrip("abcdefghijklmnopqrstuvwxyz") in [str(L) for L in EXTRA_LENGTHS]:   # "en64", "ja300", ...
            out += [(i, f) for f in EXTRA_FREQS]
    return out


@functools.lru_cache(maxsize=None)
def golden():
    """{(sentence index, freq): (Z bits, viterbi nodes, ids int64[k], reference float32[k])}."""
    g = np.load(GOLDEN)
    off = g["offsets"].astype(np.int64)
    out = {}
    for k, (s, f) in enumerate(zip(g["sentence"].tolist(), g["freq"].tolist())):
        out[(s, f)] = (int(g["z_bits"][k]), int(g["viterbi_nodes"][k]), g["ids"][off[k]:off[k + 1]].astype(np.int64),
                       g["value_bits"][off[k]:off[k + 1]].view(F))
    return out
