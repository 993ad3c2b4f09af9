"""SampleEncode's DISTRIBUTION, pinned by exact lattice marginals (emulated and -m gpu).

Lattice::Sample draws a segmentation with probability exp(theta * score) / Z.  tests/latticeref.py computes, in float64
and for one sentence of any length, the probability that an edge (begin, end) of the lattice is on the drawn path; N
copies of the sentence are sampled in one batch and every edge's count is held to

    |count - N p| <= 5 sqrt(N p (1 - p))       where N p (1 - p) >= 25        (the z-rule)
    count <= N p + 5 sqrt(N p) + 5             for the other edges            (the rare-edge rule)

5 sigma two-sided is 5.7e-7 an edge, about 10^4 edge tests in the file: under 1 % of a false alarm for a correct
sampler, and the seeds are fixed.  Every sampled span must BE an edge of the lattice, with that edge's id, and the spans
of a sample must tile the sentence (exact).  With theta <= 0.2 at least half of the edges fall under the z-rule, at
theta = 1 at least a tenth (the share is printed).  The power check: the z-rule must REJECT the marginals of the wrong
temperature 1.25 theta (theta + 0.05 at 0), in every case but one kind -- at theta = 8, where the best path holds 0.999
of the mass, no edge is left to measure, and there at least 99 % of the draws must be the oracle's Encode.

N per device-form length: 2048 up to 100 bytes, 1024 up to 400, 512 above; twice that at theta = 1; 8192 for the
sentence of one character; three cases (N_RAISED) have theirs raised until the z-rule rejects the wrong temperature.

Lengths sit around the capacities of the first lattice launch (1024 normalized bytes in DEVICE form, U+2581 one byte):
1023 / 1024 run there, 1025 and 6000 are set aside by length and run in the 32-bit-index wide launch.  "㍿" * 40 (120 raw
bytes, 481 normalized) and "㌀㍿" * 14 (84, 337) among short sentences outgrow the batch's guess (1.25 * longest raw +
16, rounded up to 64: 192 / 128) and are set aside too.  Neither LastProfile() nor the call exposes that the wide launch
ran: the lengths against the documented capacities are what says so.  A sentence set aside by node count does not
exist below 1024 bytes for the committed models: a position starts at most 8 nodes under uni32k (its deepest chain of
pieces that are prefixes of one another is 7), 1026 * 8 + 2 = 8210 nodes against the first launch's 16384.

latticeref itself is pinned first, without device code: against exp(theta * score) / Z over the oracle's enumeration,
against the oracle's Encode (the best path, for every sentence of this file) and against the compiled reference's own
sampler under the same z-rule.

Largest z seen per case (fixed seeds; the MI355X drew what the emulator drew, sample for sample, so one column), with
the share of the edges under the z-rule and the z that the wrong temperature scored.  Largest of all: 3.83.  The
compiled reference's sampler, which cannot be seeded, showed 3.62 at most over its nine cases.

    case                  theta: max z / share / z at the wrong temperature
    test_model a (2 B)    0: 0.42 / 100 % / 9.19    0.2: 0.65 / 100 % / 8.83    1: 0.64 / 100 % / 13.90   8: all 8192 draws Encode
    test_model 63 B       0.2: 2.35 / 89 % / 17.42
    test_model 64 B       0: 2.11 / 89 % / 14.62    0.2: 2.08 / 88 % / 18.49    1: 2.20 / 21 % / 13.62    8: all 2048 draws Encode
    test_model 65 B       0.2: 2.04 / 89 % / 20.34
    test_model 301 B      0: 3.15 / 93 % / 13.38    0.2: 3.04 / 90 % / 13.70    1: 2.02 / 23 % / 8.55
    test_model 1023 B     0.2: 3.83 / 83 % / 10.47
    test_model 1024 B     0.2: 3.60 / 83 % / 10.87
    test_model 1025 B     0: 3.45 / 95 % / 15.00    0.2: 3.13 / 84 % / 11.58    1: 2.57 / 12 % / 7.76     8 (N 4096): 2.31 over 23 edges / 10.34
    test_model 6000 B     0.2: 3.80 / 84 % / 11.21
    test_ja_model 61 B    0: 1.37 / 63 % / 8.12     0.2: 1.34 / 63 % / 6.96     1: 1.30 / 52 % / 10.08
    test_ja_model 302 B   0.2: 2.66 / 62 % / 6.40
    "㍿" * 40 (481 B)     0: 2.47 / 100 % / 12.87
    "㌀㍿" * 14 (337 B)   0.2 (N 2048): 2.50 / 75 % / 11.97
    uni1k_bf 64 B         0: 2.59 / 81 % / 9.47     0.2: 1.93 / 81 % / 15.15    1: 2.26 / 35 % / 11.76    8: 2047 of 2048 draws Encode
    uni1k_bf 1025 B       0.2: 3.08 / 78 % / 10.58
    uni1k_uds 100 B       0: 2.12 / 95 % / 21.38    0.2: 2.86 / 89 % / 15.28    1: 1.29 / 14 % / 11.91
    uni32k 301 B          0: 3.69 / 95 % / 19.24    0.2: 2.83 / 94 % / 9.24     1: 2.41 / 52 % / 13.19    8 (N 2048): 1.49 over 42 edges / 8.03
    uni32k 1025 B         0.2: 3.56 / 91 % / 7.88

The test has teeth beyond the power check: with alpha[pos] made to read alpha[pos - 1] for pos > 1024 in a scratch copy
of the kernel, the 6000-byte case fails at z = 81.7 (1644 rare-edge violations); the 1025-byte cases do not see that
one -- only alpha[len] itself moves there, the Z of the first draw, which scales all of its weights alike.
"""
import collections
import functools
import math
import zlib

import numpy as np
import pytest

from tests import fixtures, latticeref
from tests.test_nbest import nbest
from tests.test_sampling import _Eng, rows

SP = b"\xe2\x96\x81"


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def emu(request):
    return _Eng(request.param)


@pytest.fixture(scope="module")
def ref():
    from tests import refshim
    if not refshim.available():
        pytest.skip("oracle/_ref/libspm_ref.so not built")
    return refshim.RefLib()


@pytest.fixture(scope="module")
def procs(emu):
    """model name -> processor of this backend, loaded once."""
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = emu.load(_blob(model))
        return cache[model]
    return get


# ------------------------------------------------------------------------------------------------- the sentences ----
def _lines(corpora, name, lo, hi):
    text, offs = corpora[name]
    tb = np.asarray(text).tobytes()
    out = [tb[int(offs[i]):int(offs[i + 1])].strip() for i in range(lo, hi)]
    return [s for s in out if s]


@functools.lru_cache(maxsize=None)
def _blob(name):
    """A fixture model; "requant": test_model with its scores rounded to 1.0 (equal scores among the n best)."""
    if name == "requant":
        from sentencepiece_amd import synth
        return synth.requantized_model(fixtures.model_blob("test_model"), 1.0)
    return fixtures.model_blob(name)


@functools.lru_cache(maxsize=None)
def _model(name):
    return latticeref.Model(_blob(name))


_ORACLES, _SENT, _LAT = {}, {}, {}


def _oracle(oracle, model):
    if model not in _ORACLES:
        _ORACLES[model] = oracle.load(_blob(model))
    return _ORACLES[model]


def dev_len(norm):
    """Length of the DEVICE form of a normalized text: U+2581 is one byte there."""
    return len(norm) - 2 * norm.count(SP)


def sentence(case, corpora, oracle):
    """(raw bytes, normalized bytes) of a case: a prefix of the kind's source text whose device form has ``target``
    bytes (the first one at least that long where no prefix hits it); a kind given as bytes is the sentence itself."""
    model, kind, target = case
    if case in _SENT:
        return _SENT[case]
    o = _oracle(oracle, model)
    if isinstance(kind, bytes):
        raw = kind
    elif kind == "a":
        raw = b"a"
    elif kind in ("long0", "long1"):                       # beyond 1024 normalized bytes, for the composition tests
        src = b" ".join(_lines(corpora, "botchan", 800, 1100))
        raw = (src[:1500] if kind == "long0" else src[2000:3537]).strip()
    elif kind == "expand":
        raw = ("㍿" * 40).encode()                                # U+337F -> four ideographs under NFKC
    elif kind == "expand2":
        raw = ("㌀㍿" * 14).encode()                             # ... and U+3300 -> four katakana
    else:
        if kind in ("en", "en_known"):
            src = b" ".join(_lines(corpora, "botchan", 300, 700))
        elif kind in ("ja", "ja_known"):
            src = b"".join(_lines(corpora, "ja", 30, 200))
        elif kind == "oov":                                # characters outside a 1k English vocabulary among the words
            words = b" ".join(_lines(corpora, "botchan", 300, 700)).split(b" ")
            extra = ["café", "東京", "☃", "naïve über", "\U0001f600"]
            src = b" ".join(w if i % 7 != 3 else extra[(i // 7) % len(extra)].encode() for i, w in enumerate(words))
        elif kind == "uds":                                # the model's user-defined symbols among the words
            words = b" ".join(_lines(corpora, "botchan", 300, 700)).split(b" ")
            extra = [b"Botchan", b"the end", b"...", b"<sep>"]
            src = b" ".join(w if i % 5 != 2 else extra[(i // 5) % len(extra)] for i, w in enumerate(words))
        if kind.endswith("_known"):                        # ... without the characters the model has no piece for
            known = _model(model).match
            src = "".join(c for c in src.decode() if c == " " or c.encode() in known).encode()
        for start in range(0, 400, 7):                     # (a prefix that ends on a word's first letter skips a length:
            part = src[start:].lstrip()                    # then from another start)
            raw = None
            for k in range(max(target - 8, 1), len(part)):    # the device form grows with the prefix: the first hit
                if part[k - 1:k] == b" " or (part[k] & 0xC0) == 0x80 or (part[0] & 0xC0) == 0x80:
                    continue                               # (no trailing space, no split character)
                d = dev_len(o.normalize(part[:k]))
                if d >= target:
                    raw = part[:k]
                    break
            if raw is not None and (d == target or target not in EXACT):
                break
        assert raw is not None and (d == target or target not in EXACT)
    _SENT[case] = (raw, o.normalize(raw))
    return _SENT[case]


def lattice(case, corpora, oracle):
    if case not in _LAT:
        _LAT[case] = latticeref.Lattice(_model(case[0]), sentence(case, corpora, oracle)[1])
    return _LAT[case]


@functools.lru_cache(maxsize=None)
def _marginals(case, theta):
    return _LAT[case].marginals(theta)


def n_for(length, theta=0.0):
    """N by device-form length.  Twice that at theta = 1 (beyond one character), where the mass has gathered on few
    paths and fewer edges reach N p (1 - p) >= 25; 8192 for a sentence of one character, whose three edges move too
    little between theta and 1.25 theta for 2048 draws to tell them apart (the power check)."""
    n = 8192 if length <= 4 else 2048 if length <= 100 else 1024 if length <= 400 else 512
    return 2 * n if theta == 1.0 and length > 4 else n


# Cases whose N by class does not let the z-rule reject the wrong temperature (its z there: 4.31, 3.18, 5.65): N raised
# until it does, with room.
N_RAISED = {(("test_ja_model", "expand2", 337), 0.2): 2048, (("test_model", "en", 1025), 8.0): 4096,
            (("uni32k", "en", 300), 8.0): 2048}


# ---------------------------------------------------------------------------------------------------- the rules ----
Z_MAX = 5.0


def z_stats(counts, p, n):
    """(largest z over the edges under the z-rule, how many those are, violations of the rare-edge rule)."""
    p = np.clip(np.asarray(p, dtype=np.float64), 0.0, 1.0)
    var = n * p * (1.0 - p)
    big = var >= 25.0
    z = np.abs(counts[big] - n * p[big]) / np.sqrt(var[big])
    rare = counts[~big] > n * p[~big] + 5.0 * np.sqrt(n * p[~big]) + 5.0
    return (float(z.max()) if len(z) else 0.0), int(big.sum()), int(rare.sum())


def wrong_theta(theta):
    return 1.25 * theta if theta > 0 else 0.05


# --------------------------------------------------------------------------------------------------- the cases ----
T_ALL = (0.0, 0.2, 1.0, 8.0)
T3 = (0.0, 0.2, 1.0)
CASES = [
    (("test_model", "a", 1), T_ALL),
    (("test_model", "en", 63), (0.2,)),
    (("test_model", "en", 64), T_ALL),
    (("test_model", "en", 65), (0.2,)),
    (("test_model", "en", 300), T3),
    (("test_model", "en", 1023), (0.2,)),
    (("test_model", "en", 1024), (0.2,)),
    (("test_model", "en", 1025), T_ALL),
    (("test_model", "en", 6000), (0.2,)),
    (("test_ja_model", "ja", 60), T3),
    (("test_ja_model", "ja", 300), (0.2,)),
    (("test_ja_model", "expand", 481), (0.0,)),
    (("test_ja_model", "expand2", 337), (0.2,)),
    (("uni1k_bf", "oov", 64), T_ALL),
    (("uni1k_bf", "oov", 1025), (0.2,)),
    (("uni1k_uds", "uds", 100), T3),
    (("uni32k", "en", 300), T_ALL),
    (("uni32k", "en", 1025), (0.2,)),
]
EXACT = {63, 64, 65, 1023, 1024, 1025}                            # test_model / uni32k: the capacity boundaries, hit exactly
FLAT = [(c, t) for c, ts in CASES for t in ts]
# the compiled reference's sampler: sentences the model covers without an unknown token
REF_CASES = [(("test_model", "en", 64), T3), (("test_model", "en", 300), (0.2,)), (("test_ja_model", "ja_known", 60), (0.2,)),
             (("uni1k_uds", "uds", 100), (0.2, 1.0)), (("uni32k", "en_known", 300), (0.2, 1.0))]


def _id(v):
    if not isinstance(v, tuple):
        return "theta%g" % v
    return "%s-%s%d" % ((v[0], v[1].decode(), len(v[1])) if isinstance(v[1], bytes) else v)


# ---------------------------------------------------------------- 2. latticeref pinned, CPU only, no device code ----
CLOSED_FORM = [("test_model", b"hello world"), ("uni1k_bf", "café ab".encode()), ("test_ja_model", "東京都に行く".encode())]
NB_SENTS = [("test_model", b"a"), ("test_model", b"hello world"), ("test_model", b"this is a test"),
            ("test_ja_model", "東京都に行く".encode()), ("requant", b"in the end it was")]
SHORT90 = ("test_model", "en", 90)                                # the composition tests' sentences
LONG = [("test_model", "long0", 0), ("test_model", "long1", 0)]
EXPANDING = ("㍿" * 40).encode()


@pytest.mark.parametrize("model,sent", CLOSED_FORM)
def test_latticeref_matches_closed_form(model, sent, oracle):
    """The path probabilities equal exp(theta * score) / Z over the oracle's full enumeration (float32 scores: 1e-5)."""
    o = _oracle(oracle, model)
    npaths, paths, scores = nbest(o.lib.oracle_nbest_encode, o.h, sent, 1000)
    assert 1 < npaths < 1000
    lat = latticeref.Lattice(_model(model), o.normalize(sent))
    for theta in (0.0, 0.2, 1.0):
        w = np.array([theta * float(s) for s in scores], dtype=np.float64)
        want = dict(zip((tuple(p) for p in paths), np.exp(w - np.logaddexp.reduce(w))))
        got = collections.defaultdict(float)
        for path, _, pr in lat.path_probabilities(theta):
            got[tuple(lat.ids_of_path(path))] += pr
        assert set(got) == set(want)
        for k, p in want.items():
            assert abs(got[k] - p) <= 1e-5 * p, (model, theta, k, got[k], p)
        # ... and the edge marginals are the sums over the paths through an edge
        m = np.zeros(len(lat))
        for path, _, pr in lat.path_probabilities(theta):
            m[list(path)] += pr
        np.testing.assert_allclose(lat.marginals(theta), m, rtol=1e-9, atol=1e-15)


EVERY_SENTENCE = list(dict.fromkeys([c for c, _ in CASES] + [c for c, _ in REF_CASES] + [SHORT90] + LONG +
                                    [("test_model", EXPANDING, 0)] + [(m, s, 0) for m, s in CLOSED_FORM + NB_SENTS]))


@pytest.mark.parametrize("case", EVERY_SENTENCE, ids=_id)
def test_latticeref_best_path_is_encode(case, corpora, oracle):
    """The highest-probability path at theta = 1 is the oracle's Encode, for every sentence this file samples: by score,
    the oracle's float32 sums may tie."""
    raw, norm = sentence(case, corpora, oracle)
    lat = lattice(case, corpora, oracle)
    if case[2] in EXACT and case[1] == "en":
        assert dev_len(norm) == case[2]
    best, path = lat.best_path()
    got = lat.scores_of_ids(_oracle(oracle, case[0]).encode(raw))
    assert got, "the oracle's Encode is no path of the lattice"
    assert abs(max(got) - best) <= 1e-5 * max(abs(best), 1.0), (case, max(got), best)


@pytest.mark.parametrize("case,theta", [(c, t) for c, ts in REF_CASES for t in ts], ids=_id)
def test_latticeref_matches_reference_sampler(case, theta, corpora, oracle, ref):
    """The compiled reference's own SampleEncode under the z-rule: latticeref and the kernel are not wrong together."""
    raw, norm = sentence(case, corpora, oracle)
    lat = lattice(case, corpora, oracle)
    assert not lat.unk_char.any()                                 # boundaries follow from the pieces' byte lengths
    r = ref.load(fixtures.model_blob(case[0]))
    n = n_for(dev_len(norm), theta)
    plen = np.array([len(p[0]) for p in lat.model.pieces], dtype=np.int64)
    counts = np.zeros(len(lat), dtype=np.int64)
    for _ in range(n):
        ids = np.asarray(r.sample_encode(raw, -1, theta), dtype=np.int64)
        ends = np.cumsum(plen[ids])
        assert int(ends[-1]) == len(norm)
        for b, e, t in zip((ends - plen[ids]).tolist(), ends.tolist(), ids.tolist()):
            k = lat.edge_of[(b, e)]
            assert int(lat.id[k]) == t
            counts[k] += 1
    z, big, rare = z_stats(counts, _marginals(case, theta), n)
    print("reference sampler %s theta %g: N %d, max z %.2f over %d of %d edges" % (_id(case), theta, n, z, big, len(lat)))
    assert z <= Z_MAX and rare == 0, (case, theta, z, rare)


# ----------------------------------------------------------------------------------------- 3. the marginals test ----
@pytest.mark.parametrize("case,theta", FLAT, ids=_id)
def test_sample_marginals(case, theta, emu, procs, corpora, oracle):
    from sentencepiece_amd import synth
    model, kind, target = case
    raw, norm = sentence(case, corpora, oracle)
    lat = lattice(case, corpora, oracle)
    h = procs(model)
    L = dev_len(norm)
    n = N_RAISED.get((case, theta), n_for(L, theta))
    if kind.startswith("expand"):                                          # among short sentences: the batch's guess is too small
        sents = [raw, b"hello", b"a b"] * n
        pick = np.arange(n) * 3
        len0 = (len(raw) + len(raw) // 4 + 16 + 63) & ~63
        assert len0 < L <= 1024
    else:
        sents = [raw] * n
        pick = np.arange(n)
        if target >= 1000:
            assert (L > 1024) == (target > 1024)                  # 1023 / 1024: first launch; 1025, 6000: the wide launch
    text, offs = synth.pack(sents)
    nt, no, _ = h.NormalizePacked(text[:len(raw)], offs[:2])
    assert nt.tobytes() == norm                                   # the device's normalized text is the lattice's
    seed = zlib.crc32(("%s %s %d %g" % (model, kind, target, theta)).encode())     # fixed, and no other case's
    ids, io, b, e, nb, ne = h.SampleSpansPacked(text, offs, -1, theta, seed)
    counts = lat.count_spans(ids, io, nb, ne, pick)               # exact: every span an edge, every sample a tiling
    p = _marginals(case, theta)
    z, big, rare = z_stats(counts, p, n)
    zw, bigw, rarew = z_stats(counts, _marginals(case, wrong_theta(theta)), n)
    share = big / len(lat)
    print("marginals %s %s theta %g: N %d, L %d, max z %.2f over %d of %d edges (%.0f %%), z at theta %g: %.2f (rare %d)"
          % (emu.kind, _id(case), theta, n, L, z, big, len(lat), 100 * share, wrong_theta(theta), zw, rarew))
    assert z <= Z_MAX, "max z %.2f over %d edges" % (z, big)
    assert rare == 0, "%d edges break the rare-edge rule" % rare
    if theta <= 0.2:
        assert share >= 0.5, "only %d of %d edges under the z-rule" % (big, len(lat))
    elif theta <= 1.0:
        assert share >= 0.1, "only %d of %d edges under the z-rule" % (big, len(lat))
    # The power check: the z-rule must reject the wrong temperature.  Waived only at theta = 8 where the best path holds
    # 0.999 of the mass -- no edge is left to measure there, and the Encode assertion below takes over.
    p_best = math.exp(lat.log_prob(lat.best_path()[1], theta)) if theta == 8.0 else 0.0
    if p_best < 0.999:
        assert zw > Z_MAX, "the wrong temperature passes too (z %.2f): N is too small" % zw
    if theta == 8.0:
        if L >= 64:                                               # LogSumExp's cut (vmax > vmin + 50) is reached: somewhere
            al = lat.forward_backward(theta)[0]                   # the terms into one position lie further apart
            v = al[lat.cb] + theta * lat.score
            assert max(float(np.ptp(v[lat.ce == q])) for q in range(1, lat.n_chars + 1)) > 50.0
        if p_best >= 0.999:
            want = _oracle(oracle, model).encode(raw).tolist()
            io64 = io.astype(np.int64)
            same = sum(ids[io64[i]:io64[i + 1]].tolist() == want for i in pick)
            print("   theta 8: %d of %d draws are Encode" % (same, n))
            assert same >= 0.99 * n


# ------------------------------------------------------------------------------------------- 4. the generators ----
def _edge_rows(io, nb, ne, n, b0, e0):
    """bool[n]: row i has the span [b0, e0)."""
    io = io.astype(np.int64)
    row_of = np.repeat(np.arange(n), io[1:] - io[:-1])
    out = np.zeros(n, dtype=bool)
    out[row_of[(nb == b0) & (ne == e0)]] = True
    return out


def test_draws_are_serially_independent(emu, procs, corpora, oracle):
    """Sentences i and i + 1, and i and i + 64 (the wave stride), draw independently: for the five edges with marginal
    closest to 1/2 the sample correlation of "edge drawn" stays within 5 / sqrt(N), 5 sigma of the correlation of N
    independent pairs."""
    from sentencepiece_amd import synth
    case, theta, n = ("test_model", "en", 64), 0.2, 2048
    raw, norm = sentence(case, corpora, oracle)
    lat = lattice(case, corpora, oracle)
    p = lat.marginals(theta)
    ids, io, b, e, nb, ne = procs(case[0]).SampleSpansPacked(*synth.pack([raw] * n), -1, theta, 77)
    for k in np.argsort(np.abs(p - 0.5))[:5]:
        assert 0.1 < p[k] < 0.9
        x = _edge_rows(io, nb, ne, n, int(lat.bb[k]), int(lat.be[k])).astype(np.float64)
        for lag in (1, 64):
            r = float(np.corrcoef(x[:-lag], x[lag:])[0, 1])
            print("serial %s edge %d p %.3f lag %d: r %.4f (bound %.4f)" % (emu.kind, k, p[k], lag, r, 5 / math.sqrt(n)))
            assert abs(r) <= 5 / math.sqrt(n), (k, lag, r)


def _composition(sample, sample_spans, short, long_, others):
    """The draw's key is (seed, sentence index) and nothing else: what else is in the batch changes no draw."""
    from sentencepiece_amd import synth
    a_sents = [short] * 200
    b_sents = list(a_sents)
    changed = dict((i, long_[j % len(long_)]) for j, i in enumerate((0, 3, 64, 65, 130, 199)))
    changed.update(zip((77, 100, 101), others))
    for i, s in changed.items():
        b_sents[i] = s
    a = rows(*sample(*synth.pack(a_sents), 5))
    b = rows(*sample(*synth.pack(b_sents), 5))
    assert len(set(map(tuple, a))) > 20                           # the draws do vary
    assert [i for i in range(200) if i not in changed and a[i] != b[i]] == []
    sp_ = sample_spans(*synth.pack(b_sents), 5)                   # the spans form draws what the ids form draws
    assert rows(sp_[0], sp_[1]) == b
    sp_ = sample_spans(*synth.pack(a_sents), 5)
    assert rows(sp_[0], sp_[1]) == a
    assert rows(*sample(*synth.pack(a_sents), 5)) == a            # the same seed reproduces, another one does not
    assert rows(*sample(*synth.pack(a_sents), 6)) != a
    # ... nor does a sentence's place among those set aside: without the first two long ones the others sit two places
    # further up the list of the wide launch, on other lanes
    c_sents = list(b_sents)
    c_sents[0] = c_sents[3] = short
    c = rows(*sample(*synth.pack(c_sents), 5))
    assert [i for i in range(200) if i not in (0, 3) and b[i] != c[i]] == []
    assert c[0] == a[0] and c[3] == a[3]
    assert len({tuple(b[i]) for i in (0, 64, 130)}) == 3          # (one long sentence at three indices: three draws)


def test_unigram_draw_ignores_batch_composition(emu, procs, corpora, oracle):
    h = procs("test_model")
    short = sentence(SHORT90, corpora, oracle)[0]
    long_ = [sentence(c, corpora, oracle)[0] for c in LONG]       # beyond 1024 normalized bytes: the wide launch, another guess
    _composition(lambda t, o, seed: h.SampleEncodePacked(t, o, -1, 0.2, seed=seed),
                 lambda t, o, seed: h.SampleSpansPacked(t, o, -1, 0.2, seed),
                 short, long_, [EXPANDING, b"", b" "])


def test_bpe_dropout_draw_ignores_batch_composition(emu, procs, corpora, oracle):
    """BPE-dropout has no closed form: no distribution claim, the generator's key only."""
    h = procs("bpe1k")
    short = sentence(SHORT90, corpora, oracle)[0]
    long_ = [sentence(c, corpora, oracle)[0] for c in LONG]
    _composition(lambda t, o, seed: h.SampleEncodePacked(t, o, -1, 0.3, seed=seed),
                 lambda t, o, seed: h.SampleSpansPacked(t, o, -1, 0.3, seed),
                 short, long_, [EXPANDING, b"", b" "])


# ------------------------------------------------------------------------------------------ 5. n-best sampling ----
@pytest.mark.parametrize("nbest_size", [2, 4, 64])
@pytest.mark.parametrize("model,sent", NB_SENTS, ids=["a", "hello", "test", "ja", "requantized"])
def test_nbest_sampling_frequencies(model, sent, nbest_size, emu, procs, oracle):
    """nbest_size > 1: one of the n best with probability exp(alpha * score) / sum over the oracle's n best, under the
    z-rule.  "a" has fewer paths than any nbest_size; under the requantized model (scores rounded to 1.0) several of the
    n best score the same."""
    from sentencepiece_amd import synth
    h, o = procs(model), _oracle(oracle, model)
    k, paths, scores = nbest(o.lib.oracle_nbest_encode, o.h, sent, nbest_size)
    assert 1 <= k <= nbest_size
    if model == "requant" and nbest_size == 64:
        assert len(set(scores.tolist())) < k                      # equal scores among the n best
    n = 2048
    text, offs = synth.pack([sent] * n)
    for alpha in (0.0, 0.5):
        w = alpha * scores.astype(np.float64)
        p = np.exp(w - np.logaddexp.reduce(w))
        got = collections.Counter(tuple(x) for x in rows(*h.SampleEncodePacked(text, offs, nbest_size, alpha, seed=31 + nbest_size)))
        assert set(got) <= {tuple(q) for q in paths}
        counts = np.array([got[tuple(q)] for q in paths], dtype=np.int64)
        z, big, rare = z_stats(counts, p, n)
        print("n-best %s %s nbest %d alpha %g: %d results, max z %.2f over %d" % (emu.kind, model, nbest_size, alpha, k, z, big))
        assert z <= Z_MAX and rare == 0, (model, sent, nbest_size, alpha, z, rare)
