"""GPUDIFF_OPT_PATH_VALUES without a GPU: the model's self-check, the host twin of kernels K21 / K22
(gpudiff_render_value_from_blob: kcp_amd/csrc/valstr.h over a host-encoded blob) against the model, and valstr.h
alone in a stand-alone host program (its own main, built with AddressSanitizer and UBSan and run directly; nothing
is loaded into Python) over valid and damaged blobs.  Every comparison is exact byte equality."""
import ctypes as C
import os
import re
import subprocess

import pytest

from kcp_amd import gpudiff as G
from oracle import gpudiff_oracle as O
from oracle import upsert_oracle as U
from tests import path_values_cases as VC
from tests import path_values_model as M
from tests.golden import fixtures as F
from tests.golden.kat_cases import cases as kat_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    src = open(os.path.join(ROOT, "include", "gpudiff.h")).read()
    return int(re.search(r"#define %s (0x[0-9a-fA-F]+|\d+)u\b" % name, src).group(1), 0)


def test_option_and_constants_equal_the_header():
    assert G.OPT_PATH_VALUES == _header_define("GPUDIFF_OPT_PATH_VALUES") == 0x80000000
    assert G.VALUE_ABSENT == _header_define("GPUDIFF_VALUE_ABSENT") == M.ABSENT == 0xFF
    assert (G.TAG_NULL, G.TAG_FALSE, G.TAG_TRUE, G.TAG_INT, G.TAG_FLOAT, G.TAG_STR, G.TAG_EOBJ, G.TAG_EARR) == \
        (O.TAG_NULL, O.TAG_FALSE, O.TAG_TRUE, O.TAG_INT, O.TAG_FLOAT, O.TAG_STR, O.TAG_EOBJ, O.TAG_EARR)
    assert G.lib().gpudiff_abi_version() == 6  # additive


def test_host_only_context_takes_the_option():
    e = G.Engine(device=G.DEVICE_NONE, flags=G.OPT_PATH_VALUES)
    st = e.path_values_stats()
    assert st.batches == 0 and st.paths == 0 and st.bytes == 0
    e.close()


# ---------------------------------------------------------------- documents
def _docs():
    """Every distinct document of the KAT cases, the golden fixtures and the edge cases that the informer decodes."""
    seen, out = set(), []
    groups = [(n, a, b) for n, a, b, _se, _st in kat_cases()]
    groups += [(n, a, b) for name in F.NAMES for n, a, b, _e in F.load(name)]
    groups += VC.ALL_CASES
    for n, a, b in groups:
        for d in (a, b):
            d = G.to_json_bytes(d)
            if d in seen or len(d) > (1 << 20) or O._nesting_bound(d) > 500:  # (the 10000-deep KATs: not decoded here)
                continue
            seen.add(d)
            try:
                obj = O.informer_decode(d)
            except O.DecodeError:
                continue
            out.append((n, d, obj))
    return out


@pytest.fixture(scope="module")
def docs():
    return _docs()


def _leaf_values(x, path, out):
    if type(x) is dict and x:
        for k, v in x.items():
            _leaf_values(v, path + (("K", k),), out)
    elif type(x) is list and x:
        for i, v in enumerate(x):
            _leaf_values(v, path + (("I", i),), out)
    else:
        out[path] = x


def _python_leaves(obj):
    """path -> the decoded Python value, for the paths spec_leaves / status_leaves name."""
    out = {}
    for k, v in obj.items():
        if k in ("metadata", "status") or v is None:
            continue
        _leaf_values(v, (("K", k),), out)
    for field in ("labels", "annotations"):
        m = O.nested_string_map(obj, "metadata", field)
        for k, v in (m or {}).items():
            out[(("K", "metadata"), ("K", field), ("K", k))] = v
    if obj.get("status") is not None:
        _leaf_values(obj["status"], (("K", "status"),), out)
    return out


# ---------------------------------------------------------------- 1. the model against go_marshal
def test_model_text_is_go_marshal_of_the_leaf(docs):
    n = 0
    for name, _d, obj in docs:
        leaves = dict(O.spec_leaves(obj))
        leaves.update(O.status_leaves(obj))
        values = _python_leaves(obj)
        assert set(values) == set(leaves), name
        for p, (tag, raw) in leaves.items():
            v = values[p]
            if type(v) is float and v == 0.0:
                v = 0.0  # the canonical value holds no negative zero
            assert M.text_of(tag, raw) == U.go_marshal(v), (name, p)
            assert M.text_of(tag, raw) != b""
            n += 1
    assert n > 50000


def test_model_pins_the_named_texts():
    got = {}
    for name, a, b in VC.ALL_CASES:
        for h, k, ot, o, nt, nw in M.values_of(a, b):
            got.setdefault(name, []).append((k, ot, o, nt, nw))
    texts = {t for rows in got.values() for r in rows for t in (r[2], r[4]) if t is not None}
    for want in (b"null", b"false", b"true", b"{}", b"[]", b"0", b"-1", b"-9223372036854775808", b"9223372036854775807",
                 b"0.5", b"1e+21", b"123456789012345680000", b"0.000001", b"1e-7", b"5e-324", b'""',
                 b'"aaaaaaa\\u003czz"', b'"aaaaaaaa\\u0001zz"', b'"aaaaaa\\u2028z"', b'"aaaaaaa\\u2029z"',
                 b'"aaaaaaa\\nzz"', b'"aaaaaaaa\\"zz"'):
        assert want in texts, want
    assert b"-0" not in texts
    rows = got["numbers"]
    assert (G.PATH_CHANGED, G.TAG_INT, b"3", G.TAG_FLOAT, b"3") in rows  # 3 -> 3.0: equal texts, the tags differ
    assert (G.PATH_CHANGED, G.TAG_FLOAT, b"0", G.TAG_FLOAT, b"1.5") in rows  # -0.0 renders 0
    absent = [r for r in got["status-absent"] if (r[0] & 3) == G.PATH_STATUS_ABSENT]
    assert absent == [(G.PATH_STATUS_ABSENT | G.PATH_REGION_STATUS, M.ABSENT, None, M.ABSENT, None)]
    removed = [r for r in got["status-absent"] if (r[0] & 3) == G.PATH_REMOVED]
    assert len(removed) == 3 and all(r[2] is not None and r[4] is None for r in removed)
    assert len(got["many-150"]) == 150
    assert len(got["arena-200"]) == 29 + 1  # every 7th of 200 members, and the sentinel (neither side has status)


# ---------------------------------------------------------------- 2. the host twin against the model
_BUF = C.create_string_buffer(1 << 20)


def _render(blob, ci, status, h):
    n, tag = C.c_size_t(0), C.c_uint8(0)
    rc = G.lib().gpudiff_render_value_from_blob(blob, C.byref(ci), status, h, C.byref(tag), C.cast(_BUF, C.c_void_p),
                                                len(_BUF), C.byref(n))
    assert rc == G.OK, rc
    return tag.value, _BUF.raw[:n.value]


def _encode(doc, bits):
    for seed in range(256):
        info, blob = G.encode_object_host(doc, seed=seed, path_hash_bits=bits)
        if info["status"] == G.TOK_OK:
            return seed, info, blob
    return None, None, None


@pytest.mark.parametrize("bits", [32, 16])
def test_host_twin_equals_the_model(docs, bits):
    mask = (1 << bits) - 1
    n = 0
    for name, d, obj in docs:
        seed, info, blob = _encode(d, bits)
        if blob is None:  # no seed makes this object's hashes unique at this width
            assert bits == 16, name
            continue
        ci = G.ObjInfo(**info)
        for status, leaves in ((0, O.spec_leaves(obj)), (1, O.status_leaves(obj))):
            assert len(leaves) == (info["stat_l"] if status else info["spec_l"])
            for p, (tag, raw) in leaves.items():
                assert _render(blob, ci, status, O.path_hash(p, seed) & mask) == (tag, M.text_of(tag, raw)), (name, p)
                n += 1
    assert n > 50000


def test_capacity_notfound_and_state():
    name, a, _b = VC.DEVICE_CASES[0]
    obj = O.informer_decode(a)
    info, blob = G.encode_object_host(a)
    p = (("K", "spec"), ("K", "len13"))
    h = O.path_hash(p) & 0xFFFFFFFF
    want = M.text_of(*O.spec_leaves(obj)[p])
    assert len(want) == 15
    assert G.render_value_from_blob(blob, info, False, h) == (G.TAG_STR, want)
    ci = G.ObjInfo(**info)
    n, tag = C.c_size_t(77), C.c_uint8(0)
    buf = C.create_string_buffer(b"#" * 32, 32)
    f = G.lib().gpudiff_render_value_from_blob
    assert f(blob, C.byref(ci), 0, h, C.byref(tag), C.cast(buf, C.c_void_p), 14, C.byref(n)) == G.E_CAPACITY
    assert n.value == 15 and tag.value == G.TAG_STR and buf.raw == b"#" * 32  # the length set, nothing written
    assert f(blob, C.byref(ci), 0, h, C.byref(tag), C.cast(buf, C.c_void_p), 15, C.byref(n)) == G.OK
    assert n.value == 15 and buf.raw == want + b"#" * 17  # no terminator
    with pytest.raises(G.GpuDiffError) as ei:
        G.render_value_from_blob(blob, info, False, h, cap=3)
    assert ei.value.code == G.E_CAPACITY and ei.value.needed == 15
    # a foreign hash, the right hash in the wrong region, a hash wider than the keys
    for status, hh in ((0, h ^ 1), (1, h), (0, h | (1 << 40))):
        assert f(blob, C.byref(ci), status, hh, C.byref(tag), C.cast(buf, C.c_void_p), 32, C.byref(n)) == G.E_NOTFOUND
        assert n.value == 0 and tag.value == G.VALUE_ABSENT
    bad = G.ObjInfo(**dict(info, status=G.TOK_SYNTAX))
    assert f(blob, C.byref(bad), 0, h, C.byref(tag), C.cast(buf, C.c_void_p), 32, C.byref(n)) == G.E_STATE
    assert f(None, C.byref(ci), 0, h, C.byref(tag), C.cast(buf, C.c_void_p), 32, C.byref(n)) == G.E_INVAL
    # an info that lies about the blob: the segment does not lie inside info.bytes
    lie = G.ObjInfo(**dict(info, spec_l=1 << 24))
    assert f(blob, C.byref(lie), 0, h, C.byref(tag), C.cast(buf, C.c_void_p), 32, C.byref(n)) == G.E_NOTFOUND


# ---------------------------------------------------------------- 3. valstr.h alone, under the sanitizers
MAIN = r'''
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "valstr.h"

using namespace gd;

static int fails = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAILED line %d: %s\n", __LINE__, #x);         \
            fails++;                                              \
        }                                                         \
    } while (0)

// the program's own float formatter (valstr.h takes it as a parameter): every float is "1.5"
struct Fmt {
    uint64_t operator()(uint64_t, uint8_t* o) const {
        if (o) memcpy(o, "1.5", 3);
        return 3;
    }
};

struct Leaf {
    uint32_t key, tag;
    std::string val;  // a string's bytes, or 8 bytes of an int / float
};

// one segment as the encoders write it: vals | keys | metas | arena (tails at 4-byte offsets, padded to 16)
static std::vector<uint8_t> segment(const std::vector<Leaf>& ls, uint32_t* ar) {
    const size_t l = ls.size();
    std::vector<uint8_t> arena;
    std::vector<uint8_t> s(16 * l, 0);
    for (size_t i = 0; i < l; i++) {
        const Leaf& f = ls[i];
        const uint32_t len = (uint32_t)f.val.size(), meta = gpudiff_meta(f.tag, len);
        memcpy(&s[8 * i], f.val.data(), len < 8 ? len : 8);
        memcpy(&s[8 * l + 4 * i], &f.key, 4);
        memcpy(&s[12 * l + 4 * i], &meta, 4);
        if (gpudiff_meta_is_long(meta)) {
            arena.insert(arena.end(), f.val.begin() + 8, f.val.end());
            arena.resize((arena.size() + 3) & ~(size_t)3, 0);
        }
    }
    arena.resize(gpudiff_arena_bytes((uint32_t)arena.size()), 0);
    *ar = (uint32_t)arena.size();
    s.insert(s.end(), arena.begin(), arena.end());
    return s;
}

struct Got {
    int rc;  // 0 ok, 1 not found, 2 unresolved
    uint32_t tag;
    std::string text;
};

// what gpudiff_render_value_from_blob does, over exactly `room` bytes on the heap (ASan watches both ends)
static Got render(const std::vector<uint8_t>& blob, size_t room, uint32_t sl, uint32_t sar, uint32_t tl, uint32_t tar,
                  bool status, uint64_t h, long forced_aoff = -1, size_t short_by = 0) {
    std::vector<uint8_t> heap(blob.begin(), blob.begin() + room);  // exactly room bytes
    Got g{1, 0xFF, ""};
    const ValSeg sg = val_seg(heap.data(), heap.size(), sl, sar, tl, tar, status);
    if (!sg.ok) return Got{2, 0xFF, ""};
    const uint32_t idx = val_find(sg, h);
    if (idx == kValNoLeaf) return g;
    const ValLeaf v = val_leaf(sg, idx, forced_aoff >= 0 ? (uint64_t)forced_aoff : val_arena_prefix(sg, idx));
    const uint64_t len = val_text_len(v, Fmt());
    if (len == kValUnresolved) return Got{2, 0xFF, ""};
    CHECK(len > 0);
    // the write pass gets exactly len - short_by bytes: it must not pass their end
    std::vector<uint8_t> out(len - short_by);
    const bool ok = val_text_write(v, out.data(), out.size(), Fmt());
    CHECK(ok == (short_by == 0));
    if (!ok) return Got{2, 0xFF, ""};
    return Got{0, v.tag, std::string(out.begin(), out.end())};
}

static std::string i64(int64_t v) { return std::string((const char*)&v, 8); }

int main() {
    const std::string long_a = std::string(6, 'a') + "\xE2\x80\xA8" + "tail<\"";  // U+2028 over the head's end
    const std::string long_b(300, 'b');
    std::vector<Leaf> spec = {{10, GPUDIFF_TAG_STR, "short"},      {20, GPUDIFF_TAG_STR, long_a},
                              {30, GPUDIFF_TAG_INT, i64(-42)},      {40, GPUDIFF_TAG_STR, long_b},
                              {50, GPUDIFF_TAG_NULL, ""},           {60, GPUDIFF_TAG_STR, "12345678"},
                              {70, GPUDIFF_TAG_STR, "1234567\xE2\x80\xA9"}, {80, GPUDIFF_TAG_FLOAT, i64(0)},
                              {90, GPUDIFF_TAG_EARR, ""},           {0xFFFFFFFFu, GPUDIFF_TAG_STR, ""}};
    std::vector<Leaf> stat = {{5, GPUDIFF_TAG_TRUE, ""}, {15, GPUDIFF_TAG_STR, std::string(9, '&')},
                              {25, GPUDIFF_TAG_INT, i64(INT64_MIN)}};
    uint32_t sar, tar;
    std::vector<uint8_t> blob = segment(spec, &sar), st = segment(stat, &tar);
    blob.insert(blob.end(), st.begin(), st.end());
    const uint32_t sl = (uint32_t)spec.size(), tl = (uint32_t)stat.size();
    const size_t room = blob.size();
    CHECK(room == gpudiff_seg_bytes(sl, sar) + gpudiff_seg_bytes(tl, tar));

    // ---- valid
    Got g = render(blob, room, sl, sar, tl, tar, false, 10);
    CHECK(g.rc == 0 && g.tag == GPUDIFF_TAG_STR && g.text == "\"short\"");
    g = render(blob, room, sl, sar, tl, tar, false, 20);
    CHECK(g.rc == 0 && g.text == "\"aaaaaa\\u2028tail\\u003c\\\"\"");
    g = render(blob, room, sl, sar, tl, tar, false, 30);
    CHECK(g.rc == 0 && g.tag == GPUDIFF_TAG_INT && g.text == "-42");
    g = render(blob, room, sl, sar, tl, tar, false, 40);
    CHECK(g.rc == 0 && g.text == "\"" + long_b + "\"");
    g = render(blob, room, sl, sar, tl, tar, false, 50);
    CHECK(g.rc == 0 && g.tag == GPUDIFF_TAG_NULL && g.text == "null");
    g = render(blob, room, sl, sar, tl, tar, false, 60);
    CHECK(g.rc == 0 && g.text == "\"12345678\"");
    g = render(blob, room, sl, sar, tl, tar, false, 70);
    CHECK(g.rc == 0 && g.text == "\"1234567\\u2029\"");
    g = render(blob, room, sl, sar, tl, tar, false, 80);
    CHECK(g.rc == 0 && g.tag == GPUDIFF_TAG_FLOAT && g.text == "1.5");
    g = render(blob, room, sl, sar, tl, tar, false, 90);
    CHECK(g.rc == 0 && g.text == "[]");
    g = render(blob, room, sl, sar, tl, tar, false, 0xFFFFFFFFull);
    CHECK(g.rc == 0 && g.text == "\"\"");
    g = render(blob, room, sl, sar, tl, tar, true, 5);
    CHECK(g.rc == 0 && g.text == "true");
    g = render(blob, room, sl, sar, tl, tar, true, 15);
    CHECK(g.rc == 0 && g.text.size() == 2 + 9 * 6 && g.text.substr(1, 6) == "\\u0026");
    g = render(blob, room, sl, sar, tl, tar, true, 25);
    CHECK(g.rc == 0 && g.text == "-9223372036854775808");
    // not found: a foreign hash, a hash of the other region, a hash wider than the keys
    CHECK(render(blob, room, sl, sar, tl, tar, false, 11).rc == 1);
    CHECK(render(blob, room, sl, sar, tl, tar, false, 15).rc == 1);
    CHECK(render(blob, room, sl, sar, tl, tar, true, 10).rc == 1);
    CHECK(render(blob, room, sl, sar, tl, tar, false, (1ull << 32) | 10).rc == 1);
    // a write pass given less room than the text never passes its end (checked inside render)
    for (uint64_t h : {10ull, 20ull, 30ull, 40ull, 50ull, 80ull})
        for (size_t cut : {1u, 2u}) CHECK(render(blob, room, sl, sar, tl, tar, false, h, -1, cut).rc == 2);

    // ---- damaged: every call ends unresolved or not found, and reads nothing outside the bytes given
    // a buffer shorter than the body: both segments need all of it
    CHECK(render(blob, room - 16, sl, sar, tl, tar, true, 15).rc == 2);
    CHECK(render(blob, gpudiff_seg_bytes(sl, sar) - 1, sl, sar, tl, tar, false, 10).rc == 2);
    CHECK(render(blob, 0, sl, sar, tl, tar, false, 10).rc == 2);
    // a truncated arena: the row says less arena than the tails need
    CHECK(render(blob, room, sl, sar - 16, tl, tar, false, 40).rc == 2);
    CHECK(render(blob, gpudiff_seg_bytes(sl, 16), sl, 16, 0, 0, false, 40).rc == 2);
    CHECK(render(blob, gpudiff_seg_bytes(sl, 0), sl, 0, 0, 0, false, 20).rc == 2);
    CHECK(render(blob, gpudiff_seg_bytes(sl, 0), sl, 0, 0, 0, false, 10).rc == 0);  // inline values need no arena
    // an arena offset past the arena, or one that leaves the tail no room
    CHECK(render(blob, room, sl, sar, tl, tar, false, 40, (long)sar + 4).rc == 2);
    CHECK(render(blob, room, sl, sar, tl, tar, false, 40, (long)sar - 8).rc == 2);
    CHECK(render(blob, room, sl, sar, tl, tar, false, 40, 1l << 40).rc == 2);
    {  // a metas length past the arena
        std::vector<uint8_t> d = blob;
        const uint32_t meta = gpudiff_meta(GPUDIFF_TAG_STR, 1u << 28);
        memcpy(&d[12 * sl + 4 * 3], &meta, 4);  // leaf 3 (key 40)
        CHECK(render(d, room, sl, sar, tl, tar, false, 40).rc == 2);
        CHECK(render(d, room, sl, sar, tl, tar, false, 70).rc == 2);  // behind it: its prefix passes the arena
        CHECK(render(d, room, sl, sar, tl, tar, false, 60).rc == 0);  // an inline value behind it needs no arena
        CHECK(render(d, room, sl, sar, tl, tar, false, 20).rc == 0);  // before it: untouched
        const uint32_t m2 = gpudiff_meta(GPUDIFF_TAG_STR, 0x1FFFFFFFu);
        memcpy(&d[12 * sl + 4 * 1], &m2, 4);
        CHECK(render(d, room, sl, sar, tl, tar, false, 20).rc == 2);
    }
    {  // a len that does not fit the tag
        std::vector<uint8_t> d = blob;
        uint32_t meta = gpudiff_meta(GPUDIFF_TAG_INT, 4);
        memcpy(&d[12 * sl + 4 * 2], &meta, 4);
        CHECK(render(d, room, sl, sar, tl, tar, false, 30).rc == 2);
        meta = gpudiff_meta(GPUDIFF_TAG_NULL, 8);
        memcpy(&d[12 * sl + 4 * 4], &meta, 4);
        CHECK(render(d, room, sl, sar, tl, tar, false, 50).rc == 2);
        meta = gpudiff_meta(GPUDIFF_TAG_FLOAT, 0);
        memcpy(&d[12 * sl + 4 * 7], &meta, 4);
        CHECK(render(d, room, sl, sar, tl, tar, false, 80).rc == 2);
    }
    // lying leaf counts: more leaves than the bytes hold, in either region; fewer (the arrays are then read at
    // the wrong places, inside the bytes: any answer but a fault)
    CHECK(render(blob, room, sl + 100, sar, tl, tar, false, 10).rc == 2);
    CHECK(render(blob, room, 0xFFFFFFFFu, 0xFFFFFFF0u, tl, tar, false, 10).rc == 2);
    CHECK(render(blob, room, sl, sar, tl + 1000, tar, true, 5).rc == 2);
    CHECK(render(blob, room, sl, sar, 0xFFFFFFFFu, 0xFFFFFFF0u, true, 5).rc == 2);
    CHECK(render(blob, room, sl, 0xFFFFFFF0u, tl, tar, true, 5).rc == 2);
    for (uint32_t l = 0; l < sl; l++)
        for (uint64_t h : {10ull, 20ull, 40ull, 70ull, 0xFFFFFFFFull}) (void)render(blob, room, l, sar, 0, 0, false, h);
    for (uint32_t l = 0; l <= sl + 2; l++)
        for (uint32_t ar = 0; ar <= sar; ar += 16)
            for (uint64_t h : {5ull, 15ull, 25ull}) (void)render(blob, room, l, ar, tl, tar, true, h);
    {  // garbage: every word of the blob set, every hash asked for
        std::vector<uint8_t> d(room, 0xFF);
        for (uint64_t h : {0ull, 10ull, 0xFFFFFFFFull}) CHECK(render(d, room, sl, sar, tl, tar, false, h).rc != 0);
        std::vector<uint8_t> z(room, 0);
        for (uint64_t h : {0ull, 10ull}) (void)render(z, room, sl, sar, tl, tar, true, h);
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
'''

SAN = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _sanitizers_link(d):
    probe = os.path.join(d, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17"] + SAN + [probe, "-o", os.path.join(d, "probe")], capture_output=True)
    return r.returncode == 0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("valstr"))
    if not _sanitizers_link(d):
        pytest.skip("g++ cannot link -fsanitize=address,undefined here: the valstr.h host program was not run")
    src = os.path.join(d, "main.cpp")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run(["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "kcp_amd", "csrc"), src, "-o",
                                                   os.path.join(d, "t")], check=True)
    return os.path.join(d, "t")


def test_valstr_over_valid_and_damaged_blobs(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert MAIN.count("CHECK(") >= 45  # the program still holds its checks
