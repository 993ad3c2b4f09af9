"""Every rule of a model's precompiled_charsmap, read straight from the serialized ModelProto: the independent statement of
what the normalizer's keys are.  Nothing here touches the product's tables (csrc/tables.cc) or the oracle; the walk knows
only the blob's layout (a 4-byte trie size, the Darts double-array units, then the NUL-terminated replacement strings).
TEST INFRASTRUCTURE ONLY.

The walk runs level by level over whole arrays: a unit c is a child of the node at position p exactly when its label
equals c ^ p (that is the test a lookup makes), so one pass over all units finds a level's children at once."""
import numpy as np

MAX_DEPTH = 16        # the built-in rule sets' longest key is 12 bytes


def _varint(b, i):
    v = s = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, i


def _fields(b):
    """(field number, wire type, value) of one serialized message; bytes for wire type 2, int otherwise."""
    for f, wt, v, _, _ in _fields_raw(b):
        yield f, wt, v


def _fields_raw(b):
    """... and the byte range [start, end) of the whole field, tag included."""
    i, n = 0, len(b)
    while i < n:
        start = i
        tag, i = _varint(b, i)
        f, wt = tag >> 3, tag & 7
        if wt == 0:
            v, i = _varint(b, i)
        elif wt == 1:
            v, i = b[i:i + 8], i + 8
        elif wt == 5:
            v, i = b[i:i + 4], i + 4
        elif wt == 2:
            ln, i = _varint(b, i)
            v, i = b[i:i + ln], i + ln
        else:
            raise ValueError("wire type %d" % wt)
        yield f, wt, v, start, i


def _put_varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def with_normalizer_flag(model_bytes, field, value):
    """The ModelProto with one bool of its normalizer_spec set (3 add_dummy_prefix, 4 remove_extra_whitespaces,
    5 escape_whitespaces): the field is appended to the spec, and the last occurrence of a scalar field is its value."""
    b = bytes(model_bytes)
    out = bytearray()
    for f, wt, v, start, end in _fields_raw(b):
        if f == 3 and wt == 2:
            v = v + _put_varint(field << 3) + _put_varint(int(bool(value)))
            out += _put_varint(3 << 3 | 2) + _put_varint(len(v)) + v
        else:
            out += b[start:end]
    return bytes(out)


def charsmap_blob(model_bytes):
    """ModelProto.normalizer_spec (field 3) . precompiled_charsmap (field 2); b"" where there is none."""
    out = b""
    for f, wt, v in _fields(bytes(model_bytes)):
        if f == 3 and wt == 2:
            for g, wt2, w in _fields(v):
                if g == 2 and wt2 == 2:
                    out = w
    return out


def rules(blob):
    """precompiled_charsmap blob -> (keys, repls): two lists of bytes, sorted by key."""
    if len(blob) <= 4:
        return [], []
    tsz = int(np.frombuffer(blob[:4], dtype="<u4")[0])
    assert tsz % 4 == 0 and 4 + tsz < len(blob)
    units = np.frombuffer(blob[4:4 + tsz], dtype="<u4").astype(np.int64)
    strings = np.frombuffer(blob[4 + tsz:], dtype=np.uint8)
    n = len(units)
    offset = (units >> 10) << ((units & 0x200) >> 6)
    label = units & 0x800000FF
    leaf = (units >> 8) & 1
    idx = np.arange(n, dtype=np.int64)
    # position a lookup stands at before it reads unit c as a child: c ^ label (labels 1..255 only; a value unit has bit 31 set)
    is_child = (label >= 1) & (label <= 255)
    parent_pos = np.where(is_child, idx ^ label, -1)
    nuls = np.flatnonzero(strings == 0)

    pos = np.array([0 ^ offset[0]], dtype=np.int64)          # positions of the current level's nodes
    keys = np.zeros((1, 0), dtype=np.uint8)
    out_k, out_r = [], []
    for depth in range(1, MAX_DEPTH + 1):
        # join the level's nodes with the child units on position.  Darts-clone shares equal subtrees between keys (the
        # array is a DAWG), so several nodes of a level may stand at one position: each gets its own copy of the children
        by_pos = np.argsort(pos, kind="stable")
        spos = pos[by_pos]
        cand = idx[parent_pos >= 0]
        lo = np.searchsorted(spos, parent_pos[cand], side="left")
        cnt = np.searchsorted(spos, parent_pos[cand], side="right") - lo
        ch = np.repeat(cand, cnt)
        if not len(ch):
            break
        first = np.repeat(lo, cnt)
        within = np.arange(len(ch)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        keys = np.concatenate([keys[by_pos[first + within]], label[ch].astype(np.uint8)[:, None]], axis=1)
        pos = ch ^ offset[ch]
        inb = pos < n
        ch, keys, pos = ch[inb], keys[inb], pos[inb]
        lf = leaf[ch] == 1
        val = units[pos[lf]] & 0x7FFFFFFF
        assert (val < len(strings)).all()
        end = nuls[np.searchsorted(nuls, val)]
        sb = strings.tobytes()
        out_k.extend(r.tobytes() for r in keys[lf])
        out_r.extend(sb[int(a):int(b)] for a, b in zip(val, end))
    else:
        raise AssertionError("charsmap trie deeper than %d bytes" % MAX_DEPTH)
    order = sorted(range(len(out_k)), key=out_k.__getitem__)
    return [out_k[i] for i in order], [out_r[i] for i in order]


_cache = {}


def model_rules(model_bytes):
    """Serialized ModelProto -> (keys, repls) of its charsmap, cached by the blob's digest (four rule sets, many models)."""
    import hashlib
    blob = charsmap_blob(model_bytes)
    d = hashlib.sha256(blob).digest()
    if d not in _cache:
        _cache[d] = rules(blob)
    return _cache[d]
