"""The reference's lattice SCORES re-stated in numpy over a ``latticeref.Lattice``: what CalculateEntropy and the scores of
SampleEncodeAndScore are compared with.  TEST INFRASTRUCTURE ONLY.

The reference (src/unigram_model.cc) computes in float32, and on long text its entropy is far from the exact one: alpha
grows with the sentence and the differences ``alpha[l] - alpha[r]`` lose their digits.  Parity with ITS number is the
contract, so this file follows its order of operations to the letter:

    ForwardAlgorithm (:200-216)   alpha[pos] = LogSumExp over the edges into pos, in insertion order (begin ascending),
                                  of float32(float32(theta * score) + alpha[begin])
    LogSumExp (:47-59)            vmax + log(exp(double(vmin - vmax)) + 1.0) in double, rounded to float32; vmax alone
                                  where vmax > vmin + 50
    CalculateEntropy (:263-291)   lp = (theta * score + alpha[begin]) - alpha[pos];  H[pos] += exp(lp) * (H[begin] + lp),
                                  every product and sum rounded to float32 on its own (no fma), std::exp(float) as
                                  ``exp32`` below; the result is -H[len]
    path score (:834-841)         float32 sum of float32(theta * score) left to right, minus alpha[len]

``exact_entropy`` is the same quantity in float64 with a stable log-sum.  The cases and sentences of
tests/golden/lattice_scores.json are defined here too, for scripts/make_lattice_score_golden.py and the tests."""
import functools
import json
import os

import numpy as np

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lattice_scores.json")
SP = b"\xe2\x96\x81"


def _libm_expf():
    """glibc's expf -- the reference's std::exp(float) -- or None where no libm offers it."""
    import ctypes
    import ctypes.util
    try:
        fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").expf
    except (OSError, AttributeError):
        return None
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return fn


_EXPF = _libm_expf()


def exp32(x):
    """std::exp(float): the platform's expf; without one, the double exp rounded to float32 (equal but for a rare last
    bit: 2 of the 260 golden entropies differ between the two, by 5.6e-7 relative at most)."""
    return F(_EXPF(float(x))) if _EXPF is not None else F(np.exp(np.float64(x)))


def lse32(x, y):
    vmin, vmax = (x, y) if x < y else (y, x)
    if vmax > F(vmin + F(50.0)):
        return vmax
    return F(np.float64(vmax) + np.log(np.exp(np.float64(F(vmin - vmax))) + 1.0))


def forward32(lat, theta):
    """alpha float32[n_chars + 1] in the reference's order and arithmetic."""
    th = F(theta)
    sc = lat.score.astype(F)
    alpha = np.zeros(lat.n_chars + 1, dtype=F)
    for p in range(1, lat.n_chars + 1):
        acc = None
        for e in lat._into[p]:
            v = F(F(th * sc[e]) + alpha[lat.cb[e]])
            acc = v if acc is None else lse32(acc, v)
        alpha[p] = acc
    return alpha


def entropy32(lat, theta, alpha=None):
    """The reference's CalculateEntropy as a float32."""
    th = F(theta)
    sc = lat.score.astype(F)
    if alpha is None:
        alpha = forward32(lat, theta)
    H = np.zeros(lat.n_chars + 1, dtype=F)
    for p in range(1, lat.n_chars + 1):
        h = F(0.0)
        for e in lat._into[p]:
            lp = F(F(F(th * sc[e]) + alpha[lat.cb[e]]) - alpha[p])
            h = F(h + F(exp32(lp) * F(H[lat.cb[e]] + lp)))
        H[p] = h
    return F(-H[lat.n_chars])


def path_score32(lat, path, theta, alpha):
    """Score of a draw: the float32 sum of theta * score over the path's edges, left to right, minus alpha[len]."""
    th = F(theta)
    s = F(0.0)
    for e in path:
        s = F(s + F(th * F(lat.score[e])))
    return F(s - alpha[lat.n_chars])


def paths_of_ids(lat, ids):
    """The paths (tuples of edge indices) whose reported ids are ``ids``: ``latticeref.Lattice.scores_of_ids`` with the
    edges kept.  More than one where unknown characters are involved; none where ``ids`` is no segmentation."""
    m, ids, found = lat.model, [int(x) for x in ids], []
    stack = [(0, 0, (), False)]                                   # character position, ids consumed, edges, inside an unknown run
    while stack:
        p, k, path, in_unk = stack.pop()
        if p == lat.n_chars:
            if k == len(ids):
                found.append(path)
            continue
        if lat.unk_char[p]:
            e = lat.edge_of[(lat.starts[p], lat.starts[p + 1])]
            raw = lat.text[lat.starts[p]:lat.starts[p + 1]]
            if m.byte_fallback:
                if [m.byte_ids.get(x) for x in ids[k:k + len(raw)]] == list(raw):
                    stack.append((p + 1, k + len(raw), path + (e,), False))
            elif in_unk:
                stack.append((p + 1, k, path + (e,), True))
            elif k < len(ids) and ids[k] == m.unk_id:
                stack.append((p + 1, k + 1, path + (e,), True))
        if k < len(ids) and ids[k] != m.unk_id:
            for e in lat._from[p]:
                if int(lat.id[e]) == ids[k]:
                    stack.append((int(lat.ce[e]), k + 1, path + (int(e),), False))
    return found


def exact_entropy(lat, theta):
    """The entropy of the path distribution exp(theta * score) / Z in float64."""
    alpha = lat.forward_backward(theta)[0]
    H = np.zeros(lat.n_chars + 1)
    for p in range(1, lat.n_chars + 1):
        e = lat._into[p]
        lp = theta * lat.score[e] + alpha[lat.cb[e]] - alpha[p]
        H[p] = float(np.sum(np.exp(lp) * (H[lat.cb[e]] + lp)))
    return float(-H[lat.n_chars])


def bits(x):
    return int(np.asarray(x, dtype=F).view(np.uint32))


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(F)


# ------------------------------------------------------------------------------------------------------ the cases ----
THETAS = (0.0, 0.2, 1.0, 8.0)
# (model, kind of text as tests/test_sampling_marginals.py builds it, device-form lengths).  63 / 64 / 65 and 1023 / 1024 /
# 1025 are hit exactly (EXACT_MODELS): the capacity of the first lattice launch is 1024 device bytes.  The Japanese text
# has ASCII letters and digits mixed in (scripts/make_lattice_score_golden.py), or its three-byte characters would skip
# two lengths of three.
SENTENCES = [
    ("test_model", "en", (1, 63, 64, 65, 300, 1023, 1024, 1025, 3000, 6000)),
    ("test_ja_model", "ja", (1, 63, 64, 65, 300, 1023, 1024, 1025, 3000, 6000)),
    ("uni1k_bf", "oov", (1, 63, 64, 65, 300, 1023, 1024, 1025, 3000, 6000)),
    ("uni1k_uds", "uds", (1, 63, 64, 65, 300, 1023, 1024, 1025, 3000, 6000)),
    ("uni32k", "en", (1, 63, 64, 65, 300, 1023, 1024, 1025, 3000, 6000)),
]
EXACT_MODELS = ("test_model", "test_ja_model", "uni1k_bf", "uni1k_uds", "uni32k")
FIXED = [("expand", ("㍿" * 40)), ("empty", ""), ("spaces", "   ")]          # under every model
# result counts of SampleEncodeAndScore without replacement (test_model): sentences with 1, 2, 7, 35 and 48 paths
COUNT_SENTENCES = ["☃", "a", "hello", "hello world", "in the end", ""]
COUNT_SAMPLES = (1, 2, 3, 8)


def dev_len(norm):
    return len(norm) - 2 * norm.count(SP)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)
