"""The charsmap sweep's inputs, built deterministically from a model's own rule keys (tests/charsmapkeys.py):
  * sentences: every key in nine contexts (CONTEXTS), context-major, so sentence i was built from key i % len(keys);
  * documents: the keys in chunks of 4 000 joined with "", " ", "a" and "  " behind 0..63 filler bytes (every phase for
    every separator), plus one concatenation above 256 KB;
  * code points: U+0001..U+10FFFF without surrogates, 512 to a sentence with "a" between them, the range below U+30000
    again one to a sentence, and every two-byte pair (b0 >= 0x80, b1) as "a" b0 b1 "a".
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

MARKS = ("́".encode(), "゙".encode(), "ﾞ".encode())     # a longer key may or may not exist behind the key

# name, what the sentence is made of
CONTEXTS = [
    ("k", lambda k: k),
    ("a k b, no spaces", lambda k: b"a" + k + b"b"),
    ("' ' k ' x'", lambda k: b" " + k + b" x"),
    ("k ' ' k", lambda k: k + b" " + k),
    ("k cut one byte short + z", lambda k: k[:-1] + b"z"),
    ("'x ' k", lambda k: b"x " + k),
    ("k + U+0301", lambda k: k + MARKS[0]),
    ("k + U+3099", lambda k: k + MARKS[1]),
    ("k + U+FF9E", lambda k: k + MARKS[2]),
]
CHUNK = 4000
SEPARATORS = (b"", b" ", b"a", b"  ")
FILLER = b"q"            # lower case: no rule set rewrites it


def pack(parts):
    lens = np.fromiter(map(len, parts), dtype=np.uint64, count=len(parts))
    offs = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    return np.frombuffer(b"".join(parts), dtype=np.uint8), offs


def is_hangul_composition(key):
    """A key of two or more characters, all of them jamo (conjoining, compatibility, half-width, enclosed) or precomposed
    syllables: nine tenths of every built-in rule set, one algorithmic family."""
    s = key.decode("utf-8")
    return len(s) >= 2 and all(0x1100 <= c <= 0x11FF or 0x3130 <= c <= 0x318F or 0x3200 <= c <= 0x321E or
                               0x3260 <= c <= 0x327F or 0xFFA0 <= c <= 0xFFDC or 0xAC00 <= c <= 0xD7A3
                               for c in map(ord, s))


def thin(keys):
    """The keys that are not Hangul compositions plus every 16th Hangul one (in key order)."""
    out, h = [], 0
    for k in keys:
        if is_hangul_composition(k):
            h += 1
            if h % 16:
                continue
        out.append(k)
    return out


class Sentences:
    """Every key in every context, context-major; with one_context, key i in context i % 9 only."""

    def __init__(self, keys, one_context=False):
        self.keys, self.one_context = keys, one_context
        if one_context:
            parts = [CONTEXTS[i % len(CONTEXTS)][1](k) for i, k in enumerate(keys)]
        else:
            parts = []
            for _, f in CONTEXTS:
                parts.extend(map(f, keys))
        self.text, self.offs = pack(parts)

    def describe(self, i):
        k = self.keys[i % len(self.keys)]
        ctx = i % len(CONTEXTS) if self.one_context else i // len(self.keys)
        return "sentence %d %r: context %r of key %r (%s)" % (
            i, self.text[int(self.offs[i]):int(self.offs[i + 1])].tobytes(), CONTEXTS[ctx][0], k,
            " ".join("U+%04X" % ord(c) for c in k.decode("utf-8")))


class Documents:
    def __init__(self, keys):
        self.keys = keys
        n = len(keys)
        chunks = max(64, -(-n // CHUNK))         # at least 64, wrapping round the key list, so that every phase occurs
        parts, self.what = [], []
        for si, sep in enumerate(SEPARATORS):
            for c in range(chunks):
                lo = c * CHUNK % n
                ks = keys[lo:lo + CHUNK]
                phase = (c + 17 * si) % 64
                parts.append(FILLER * phase + sep.join(ks))
                self.what.append("keys[%d:%d] joined with %r behind %d filler bytes" % (lo, lo + len(ks), sep, phase))
        big, size = [], 0
        for k in keys:                           # the few-long-documents form: one text above 256 KB
            big.append(k)
            size += len(k) + 1
            if size > 300 * 1024:
                break
        parts.append(b" ".join(big))
        self.what.append("keys[0:%d] joined with ' '" % len(big))
        self.text, self.offs = pack(parts)

    def describe(self, i):
        return "document %d (%d bytes): %s" % (i, int(self.offs[i + 1] - self.offs[i]), self.what[i])


class CodePoints:
    def __init__(self):
        cps = [c for c in range(1, 0x110000) if not 0xD800 <= c < 0xE000]
        enc = [chr(c).encode("utf-8") for c in cps]
        parts = [b"a".join(enc[i:i + 512]) for i in range(0, len(enc), 512)]
        self.what = ["U+%04X.. 512 code points joined with 'a'" % cps[i] for i in range(0, len(enc), 512)]
        self.n_packed = len(parts)
        single = [e for c, e in zip(cps, enc) if c < 0x30000]
        self.single_cps = [c for c in cps if c < 0x30000]
        parts.extend(single)
        self.n_single = len(single)
        parts.extend(b"a" + bytes((b0, b1)) + b"a" for b0 in range(0x80, 0x100) for b1 in range(0x100))
        self.text, self.offs = pack(parts)

    def describe(self, i):
        b = self.text[int(self.offs[i]):int(self.offs[i + 1])].tobytes()
        if i < self.n_packed:
            return "sentence %d: %s" % (i, self.what[i])
        if i < self.n_packed + self.n_single:
            return "sentence %d %r: U+%04X alone" % (i, b, self.single_cps[i - self.n_packed])
        return "sentence %d %r: a two-byte pair between 'a's" % (i, b)


@functools.lru_cache(maxsize=1)
def code_points():
    return CodePoints()


def first_difference(got, want, got_offs=None, want_offs=None):
    """Index of the first sentence whose slice of two CSR results differs, or None.  Without offsets: index of the first
    differing element."""
    got, want = np.asarray(got), np.asarray(want)
    if got_offs is not None:
        go, wo = np.asarray(got_offs).astype(np.int64), np.asarray(want_offs).astype(np.int64)
        if len(go) != len(wo):
            return 0
        d = np.flatnonzero(go != wo)
        first_off = int(d[0]) - 1 if len(d) else None       # sentence whose END moved
    else:
        first_off = None
    m = min(len(got), len(want))
    d = np.flatnonzero(got[:m].astype(np.int64) != want[:m].astype(np.int64))
    first_el = int(d[0]) if len(d) else (m if len(got) != len(want) else None)
    if got_offs is None:
        return first_el
    if first_el is not None:
        s = int(np.searchsorted(wo, first_el, side="right")) - 1
        first_off = s if first_off is None else min(first_off, s)
    return None if first_off is None else max(first_off, 0)
