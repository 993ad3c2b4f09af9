"""SampleEncodeAndScore on the device (kernels_nbest.h modes 4 and 5), emulated and -m gpu.

With replacement   every score is the reference's number for the returned path: the float32 sum of theta * score minus
                   alpha[len] of tests/latticescore.py (bit-equal emulated, 2e-4 relative + 1e-6 on the MI355X, the
                   bounds of tests/test_entropy.py); the draws follow the lattice's edge marginals under the z-rule of
                   tests/test_sampling_marginals.py and are keyed by (hash of the seed, sentence, draw) alone.
Without            the rows of a sentence are distinct paths; the result counts are the compiled reference's
replacement        (tests/golden/lattice_scores.json), its "P - 1 results for P <= num_samples paths" included; the
                   paths are drawn with the inclusion probabilities of successive sampling without replacement
                   (enumerated exactly), and the scores obey the reference's own identity (unigram_model_test.cc:594-609,
                   arXiv 1903.06059 appendix D): E[1{path drawn} exp(-score)] = 1.

Seen (fixed seeds; the MI355X drew what the emulator drew): with-replacement scores 96 of 96 bit-equal on both; pooled
marginals max z 3.89 / 4.41 (18.74 / 14.53 at the wrong temperature; these two seeds sit high, twelve other seeds gave
2.21 - 3.01 and 2.72 - 4.27); without replacement max z 2.79 over the twelve cases, the identity within 2.84 standard
errors at most, 5.84 at least with 1 / pi of the wrong temperature.
"""
import collections
import math
import zlib

import numpy as np
import pytest

from tests import fixtures, latticeref, latticescore as ls
from tests.test_entropy import RTOL, ATOL, cases_of
from tests.test_sampling import _Eng, rows
from tests.test_sampling_marginals import EXPANDING, Z_MAX, _composition, wrong_theta, z_stats


@pytest.fixture(scope="module", params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def emu(request):
    return _Eng(request.param)


@pytest.fixture(scope="module")
def procs(emu):
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = emu.load(fixtures.model_blob(model))
        return cache[model]
    return get


_LAT = {}


def lattice(model, raw, oracle):
    if (model, raw) not in _LAT:
        o = oracle.load(fixtures.model_blob(model))
        _LAT[(model, raw)] = latticeref.Lattice(latticeref.Model(fixtures.model_blob(model)), o.normalize(raw))
    return _LAT[(model, raw)]


def golden_raw(model, name):
    (s,) = [s for s, _ in cases_of(model) if s["name"] == name]
    return s["raw"].encode()


def by_sentence(ids, io, ro):
    """The CSR of results -> one row per SENTENCE (its results' ids in a row, a -1 between them): what _composition compares."""
    io, ro = io.astype(np.int64), ro.astype(np.int64)
    out, offs = [], [0]
    for s in range(len(ro) - 1):
        for r in range(ro[s], ro[s + 1]):
            out += ids[io[r]:io[r + 1]].tolist() + [-1]
        offs.append(len(out))
    return np.asarray(out, dtype=np.int32), np.asarray(offs, dtype=np.uint64)


def row_paths(lat, res, rows_):
    """Edge sets of the rows ``rows_`` of a spans-form result: count_spans asserts that each tiles the sentence with edges."""
    ids, io, sc, ro, b, e, nb, ne = res
    out = []
    for r in rows_:
        c = lat.count_spans(ids, io, nb, ne, [r])
        assert c.max() == 1
        out.append(tuple(np.flatnonzero(c).tolist()))
    return out


# ------------------------------------------------------------------------------------ 1. with replacement: scores ----
@pytest.mark.parametrize("model,kind", [("test_model", "en"), ("uni1k_bf", "oov"), ("uni32k", "en")])
def test_wr_scores_are_the_reference_numbers(model, kind, emu, procs, oracle):
    """Every row: score == float32 path score - alpha32[len] of the returned ids.  64 bytes, the capacity boundary
    1024 / 1025 and the wide launch's 3000; on uni1k_bf's text with unknown characters any matching path is accepted."""
    from sentencepiece_amd import synth
    h = procs(model)
    raws = [golden_raw(model, "%s%d" % (kind, L)) for L in (64, 1024, 1025, 3000)]
    text, offs = synth.pack(raws)
    worst, equal, total = 0.0, 0, 0
    for theta in (0.2, 1.0):
        ids, io, sc, ro = h.SampleEncodeAndScorePacked(text, offs, 4, theta, seed=11)
        assert ro.tolist() == [0, 4, 8, 12, 16]
        io = io.astype(np.int64)
        for s, raw in enumerate(raws):
            lat = lattice(model, raw, oracle)
            alpha = ls.forward32(lat, theta)
            for r in range(4 * s, 4 * s + 4):
                row = ids[io[r]:io[r + 1]].tolist()
                paths = ls.paths_of_ids(lat, row)
                assert paths, "the returned ids are no path of the lattice"
                assert len(lat.scores_of_ids(row)) == len(paths)
                want = [ls.path_score32(lat, p, theta, alpha) for p in paths]
                total += 1
                equal += any(ls.bits(w) == ls.bits(sc[r]) for w in want)
                err = min(abs(float(sc[r]) - float(w)) - (RTOL * abs(float(w)) + ATOL) for w in want)
                worst = max(worst, min(abs(float(sc[r]) - float(w)) / abs(float(w)) for w in want))
                if emu.kind == "emu":
                    assert any(ls.bits(w) == ls.bits(sc[r]) for w in want), (model, theta, s, float(sc[r]), [float(w) for w in want])
                else:
                    assert err <= 0.0, (model, theta, s, float(sc[r]), [float(w) for w in want])
    print("wr scores %s %s: %d of %d bit-equal, largest relative difference %.3g" % (emu.kind, model, equal, total, worst))


# ------------------------------------------------------------------------------ 2. with replacement: distribution ----
WR_CASES = [("test_model", "en64"), ("uni32k", "en300")]


@pytest.mark.parametrize("model,name", WR_CASES)
def test_wr_draws_follow_the_marginals(model, name, emu, procs, oracle):
    """The num_samples = 4 draws of N = 512 copies, pooled, under the z-rule at theta 0.2; the wrong temperature is
    rejected; draws j and j + 1 of one sentence are uncorrelated (5 / sqrt(N) on the five edges nearest p = 1/2)."""
    from sentencepiece_amd import synth
    h, theta, n, k = procs(model), 0.2, 512, 4
    raw = golden_raw(model, name)
    lat = lattice(model, raw, oracle)
    seed = zlib.crc32(("wr %s %s" % (model, name)).encode())
    res = h.SampleEncodeAndScorePacked(*synth.pack([raw] * n), k, theta, seed=seed, spans=True)
    ids, io, sc, ro, b, e, nb, ne = res
    assert ro.tolist() == list(range(0, k * n + 1, k))
    counts = lat.count_spans(ids, io, nb, ne, np.arange(k * n))
    p = lat.marginals(theta)
    z, big, rare = z_stats(counts, p, k * n)
    zw, _, rarew = z_stats(counts, lat.marginals(wrong_theta(theta)), k * n)
    print("wr marginals %s %s %s: N %d x %d, max z %.2f over %d of %d edges, z at theta %g: %.2f (rare %d)"
          % (emu.kind, model, name, n, k, z, big, len(lat), wrong_theta(theta), zw, rarew))
    assert z <= Z_MAX and rare == 0, (z, rare)
    assert zw > Z_MAX, "the wrong temperature passes too (z %.2f)" % zw
    io64 = io.astype(np.int64)
    row_of = np.repeat(np.arange(k * n), io64[1:] - io64[:-1])
    for edge in np.argsort(np.abs(p - 0.5))[:5]:
        assert 0.1 < p[edge] < 0.9
        x = np.zeros(k * n)
        x[row_of[(nb == lat.bb[edge]) & (ne == lat.be[edge])]] = 1.0
        x = x.reshape(n, k)
        for j in range(k - 1):
            r = float(np.corrcoef(x[:, j], x[:, j + 1])[0, 1])
            print("   edge %d p %.3f draws %d, %d: r %.4f (bound %.4f)" % (edge, p[edge], j, j + 1, r, 5 / math.sqrt(n)))
            assert abs(r) <= 5 / math.sqrt(n), (edge, j, r)


# SampleEncodePacked(64 copies of the composition test's short sentence, -1, 0.2, seed 5) as the commit BEFORE the scored
# entry points drew it under the emulator, which is what the MI355X draws too: the sampler they now share draws what it drew
SAMPLE_ENCODE_PIN = 0x9EC3B462


def test_wr_keys(emu, procs, corpora, oracle):
    """Draw j of sentence i is keyed by (seed, i, j) alone: the same seed reproduces, another does not, what else is in
    the batch changes no draw (the _composition pattern of the marginals test), the spans form draws the same -- and
    SampleEncode's own draws are what they were."""
    from tests.test_sampling_marginals import LONG, SHORT90, sentence
    h = procs("test_model")
    short = sentence(SHORT90, corpora, oracle)[0]
    long_ = [sentence(c, corpora, oracle)[0] for c in LONG]

    def sample(t, o, seed):
        ids, io, sc, ro = h.SampleEncodeAndScorePacked(t, o, 2, 0.2, seed=seed)
        return by_sentence(ids, io, ro)

    def sample_spans(t, o, seed):
        res = h.SampleEncodeAndScorePacked(t, o, 2, 0.2, seed=seed, spans=True)
        return by_sentence(res[0], res[1], res[3])
    _composition(sample, sample_spans, short, long_, [EXPANDING, b"", b" "])
    # the two draws of a sentence differ from one another somewhere, and from SampleEncode's draw with that seed
    from sentencepiece_amd import synth
    text, offs = synth.pack([short] * 64)
    ids, io, sc, ro = h.SampleEncodeAndScorePacked(text, offs, 2, 0.2, seed=5)
    r = rows(ids, io)
    assert sum(r[2 * i] != r[2 * i + 1] for i in range(64)) > 32
    plain = rows(*h.SampleEncodePacked(text, offs, -1, 0.2, seed=5))
    assert rows(*h.SampleEncodePacked(text, offs, -1, 0.2, seed=5)) == plain
    crc = zlib.crc32(repr(plain).encode())
    print("SampleEncodePacked pin %s: %#x" % (emu.kind, crc))
    assert crc == SAMPLE_ENCODE_PIN


# ------------------------------------------------------------------------------- 3. without replacement: structure ----
def test_wor_result_counts_are_the_reference_counts(emu, procs, oracle):
    """num_samples 1, 2, 3, 8 with and without include_best on sentences with 1, 2, 7, 35 and 48 paths and an empty one:
    the compiled reference's counts.  One path or none: no result for THAT sentence (the per-sentence INTERNAL status);
    the single call with it raises.  Rows are distinct paths; with include_best row 0 is Encode with score exactly 0."""
    from sentencepiece_amd import synth
    h, model = procs("test_model"), "test_model"
    o = oracle.load(fixtures.model_blob(model))
    sents = [s.encode() for s in ls.COUNT_SENTENCES]
    lats = [lattice(model, s, oracle) for s in sents]
    assert [len(lat.paths()) if lat.n_chars else 0 for lat in lats] == [1, 2, 7, 35, 48, 0]
    want = collections.defaultdict(dict)
    for c in ls.golden()["wor_counts"]:
        assert c["paths"] == (len(lats[ls.COUNT_SENTENCES.index(c["raw"])].paths()) if c["raw"] else 0)
        # -1: the reference's "returns empty result."; null: it reads an empty vector there (one path, include_best)
        want[(c["num_samples"], c["include_best"])][c["raw"]] = max(c["results"], 0) if c["results"] is not None else 0
    text, offs = synth.pack(sents)
    for (num, best), per in sorted(want.items()):
        res = h.SampleEncodeAndScorePacked(text, offs, num, 1.0, wor=True, include_best=bool(best), seed=num, spans=True)
        ids, io, sc, ro = res[:4]
        ro = ro.astype(np.int64)
        assert (ro[1:] - ro[:-1]).tolist() == [per[s] for s in ls.COUNT_SENTENCES], (num, best)
        r = rows(ids, io)
        for i, (s, lat) in enumerate(zip(sents, lats)):
            mine = list(range(ro[i], ro[i + 1]))
            paths = row_paths(lat, res, mine)
            assert len(set(paths)) == len(paths), "a path twice among the rows of a sentence"
            if best and mine:
                assert r[mine[0]] == o.encode(s).tolist() and ls.bits(sc[mine[0]]) == 0
            assert all(float(x) <= 0.0 for x in sc[mine])                      # log probabilities
    assert want[(3, 0)]["a"] == 1                                 # the reference's quirk: 2 paths, 3 samples, ONE result
    for s in ("☃", ""):
        with pytest.raises(RuntimeError, match="SampleEncodeAndScore returns empty result."):
            h.SampleEncodeAndScore(s, num_samples=2, alpha=1.0, wor=True, seed=1)
    with pytest.raises(RuntimeError, match="SampleEncodeAndScore returns empty result."):
        h.SampleEncodeAndScore(["hello", ""], num_samples=2, alpha=1.0, seed=1)


def test_wor_in_the_wide_launch(emu, procs, oracle):
    """1025 and 3000 device bytes (beyond the first launch) with num_samples = 4, with and without include_best:
    distinct lattice paths, and the draws do not depend on what else is in the batch."""
    from sentencepiece_amd import synth
    h, model = procs("test_model"), "test_model"
    raws = [golden_raw(model, "en1025"), golden_raw(model, "en3000"), b"hello world"]
    res = h.SampleEncodeAndScorePacked(*synth.pack(raws), 4, 0.5, wor=True, include_best=True, seed=9, spans=True)
    assert res[3].tolist() == [0, 4, 8, 12]                       # the best path and three samples (:775-798)
    for i, raw in enumerate(raws):
        paths = row_paths(lattice(model, raw, oracle), res, range(4 * i, 4 * i + 4))
        assert len(set(paths)) == 4
    plain = h.SampleEncodeAndScorePacked(*synth.pack(raws), 4, 0.5, wor=True, seed=9, spans=True)
    assert plain[3].tolist() == [0, 4, 8, 12]
    for i, raw in enumerate(raws):
        assert len(set(row_paths(lattice(model, raw, oracle), plain, range(4 * i, 4 * i + 4)))) == 4
    alone = h.SampleEncodeAndScorePacked(*synth.pack([b"a b", raws[1], b"c"]), 4, 0.5, wor=True, include_best=True, seed=9)
    # (the key is (seed, sentence index): the 3000-byte sentence sits at index 1 in both batches)
    r0, r1 = int(alone[3][1]), int(alone[3][2])
    assert r1 - r0 == 4 and rows(alone[0], alone[1])[r0:r1] == rows(res[0], res[1])[4:8]
    assert np.array_equal(alone[2][r0:r1].view(np.uint32), res[2][4:8].view(np.uint32))


# -------------------------------------------------------------- 4. without replacement: inclusion probabilities ----
def inclusion_probabilities(p, k):
    """P(path i is among the first k of successive draws without replacement, each proportional to p among the paths
    left): what Gumbel top-k draws.  Exact enumeration, at most len(p)^3 terms."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    out = p.copy()
    if k >= 2 and n >= 2:
        first = p[:, None]                                        # j first, then i
        second = p[None, :] / (1.0 - p[:, None])
        m2 = first * second
        np.fill_diagonal(m2, 0.0)
        out = out + m2.sum(axis=0)
    if k >= 3 and n >= 3:
        pj, pl, pi = p[:, None, None], p[None, :, None], p[None, None, :]
        den = 1.0 - pj - pl
        with np.errstate(divide="ignore", invalid="ignore"):
            m3 = pj * (pl / (1.0 - pj)) * (pi / den)
        idx = np.arange(n)
        m3[idx, idx, :] = 0.0
        m3[idx, :, idx] = 0.0
        m3[:, idx, idx] = 0.0
        out = out + m3.sum(axis=(0, 1))
    assert k <= 3
    return np.minimum(out, 1.0) if k < n else np.ones(n)


def test_inclusion_probabilities_helper():
    p = np.array([0.5, 0.3, 0.2])
    assert np.allclose(inclusion_probabilities(p, 1), p)
    assert np.allclose(inclusion_probabilities(p, 3), 1.0)
    pi2 = inclusion_probabilities(p, 2)
    assert abs(pi2.sum() - 2.0) < 1e-12                           # k paths are drawn
    assert abs(pi2[0] - (0.5 + 0.3 * 0.5 / 0.7 + 0.2 * 0.5 / 0.8)) < 1e-12
    q = np.random.RandomState(3).dirichlet(np.ones(9))
    for k in (1, 2, 3):
        assert abs(inclusion_probabilities(q, k).sum() - k) < 1e-9


N_WOR = 4096


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("theta", [0.0, 1.0])
@pytest.mark.parametrize("sent", [b"hello", b"in the end"])
def test_wor_inclusion_probabilities_and_scores(sent, theta, k, emu, procs, oracle):
    """N = 4096 copies in one batch.  The count of copies that drew a path obeys the z-rule and the rare-path rule
    against the exact inclusion probability; for every path with N pi >= 100 the mean of 1{drawn} exp(-score) is 1
    within 5 of its own standard errors.  Power: 1 / pi of the wrong temperature in place of exp(-score) fails that, and
    at num_samples = 3 the counts reject the with-replacement probabilities 1 - (1 - p)^3.

    Two cases cannot carry a part of this, by the exact probabilities alone: "in the end" at theta 0 has 48 equally likely
    paths, so at k = 1 no path reaches N pi >= 100 (4096 / 48 = 85) and the identity has nothing to test; and at k = 3 its
    inclusion probability 3 / 48 = 0.0625 lies 0.35 sigma from 1 - (47 / 48)^3 = 0.0612 at N = 4096, which no count can
    tell apart.  The with-replacement check is therefore asserted where the exact probabilities put the two hypotheses
    at least 7 sigma apart in some path (7.7 for "hello" at theta 0, hundreds at theta 1)."""
    from sentencepiece_amd import synth
    h, n = procs("test_model"), N_WOR
    lat = lattice("test_model", sent, oracle)
    pp = lat.path_probabilities(theta)
    index = {tuple(lat.ids_of_path(path)): i for i, (path, _, _) in enumerate(pp)}
    assert len(index) == len(pp) in (7, 48)
    p = np.array([q for _, _, q in pp])
    pi = inclusion_probabilities(p, k)
    seed = zlib.crc32(("wor %s %g %d" % (sent.decode(), theta, k)).encode())
    ids, io, sc, ro = h.SampleEncodeAndScorePacked(*synth.pack([sent] * n), k, theta, wor=True, seed=seed)
    assert ro.tolist() == list(range(0, k * n + 1, k))
    which = np.array([index[tuple(r)] for r in rows(ids, io)]).reshape(n, k)
    assert all(len(set(w)) == k for w in which.tolist())          # distinct within a sentence
    counts = np.bincount(which.ravel(), minlength=len(p))
    z, big, rare = z_stats(counts, pi, n)
    # 1{drawn} exp(-score) per copy and path
    val = np.zeros((n, len(p)))
    val[np.repeat(np.arange(n), k), which.ravel()] = np.exp(-sc.astype(np.float64))
    pw = inclusion_probabilities(np.array([q for _, _, q in lat.path_probabilities(wrong_theta(theta))]), k)
    worst = worst_wrong = 0.0
    tested = 0
    for i in np.flatnonzero(n * pi >= 100):
        v = val[:, i]
        se = v.std(ddof=1) / math.sqrt(n)
        dev = abs(v.mean() - 1.0) / se if se > 0 else (0.0 if v.mean() == 1.0 else math.inf)
        w = (val[:, i] > 0) / pw[i]
        sew = w.std(ddof=1) / math.sqrt(n)
        devw = abs(w.mean() - 1.0) / sew if sew > 0 else (0.0 if w.mean() == 1.0 else math.inf)
        worst, worst_wrong, tested = max(worst, dev), max(worst_wrong, devw), tested + 1
    print("wor %s %s theta %g k %d: max z %.2f over %d of %d paths (rare %d); identity within %.2f se over %d paths, wrong "
          "temperature %.2f se" % (emu.kind, sent.decode(), theta, k, z, big, len(p), rare, worst, tested, worst_wrong))
    assert z <= Z_MAX and rare == 0, (z, rare)
    assert worst <= 5.0
    assert tested > 0 or (sent, theta, k) == (b"in the end", 0.0, 1)
    if tested:
        assert worst_wrong > 5.0, "1 / pi of the wrong temperature passes the identity too"
    if k == 3:
        pwr = 1.0 - (1.0 - p) ** 3
        apart = float(np.max(n * np.abs(pi - pwr) / np.sqrt(n * pwr * (1.0 - pwr))))
        zr = z_stats(counts, pwr, n)[0]
        print("   against the with-replacement probabilities: z %.2f (%.1f sigma apart)" % (zr, apart))
        assert apart >= 7.0 or (sent, theta) == (b"in the end", 0.0)
        if apart >= 7.0:
            assert zr > Z_MAX


# ------------------------------------------------------------------------------------------------- 5. the statuses ----
def test_statuses(emu, procs):
    from sentencepiece_amd import synth
    h = procs("test_model")
    text, offs = synth.pack([b"hello world"])
    for kw, msg in ((dict(num_samples=2, include_best=True), "SampleEncodeAndScore returns empty result."),
                    (dict(num_samples=0), "SampleEncodeAndScore returns empty result."),
                    (dict(num_samples=0, wor=True), "SampleEncodeAndScore returns empty result."),
                    (dict(num_samples=513), "num_samples must be num_samples <= 512"),
                    (dict(num_samples=513, wor=True), "num_samples must be num_samples <= 512")):
        with pytest.raises(RuntimeError, match=msg):
            h.SampleEncodeAndScorePacked(text, offs, alpha=0.5, **kw)
    assert len(h.SampleEncodeAndScorePacked(text, offs, 512, 0.5)[2]) == 512
    # the Python entry refuses these itself, in the wheel's words
    with pytest.raises(RuntimeError, match='When include_best is True, We must specify "wor = True".'):
        h.SampleEncodeAndScore("hello", num_samples=2, include_best=True)
    with pytest.raises(RuntimeError, match="num_examples must be positive"):
        h.SampleEncodeAndScore("hello", num_samples=0)
    for model in ("bpe1k", "char1k", "word1k"):
        other = emu.load(fixtures.model_blob(model))
        with pytest.raises(RuntimeError, match="SampleEncodeAndScore is not available for the current model."):
            other.SampleEncodeAndScore("hello", num_samples=2, alpha=0.5)
