// Rendering one leaf's value as JSON text from the segments a blob carries
// (include/gpudiff_format.h): the one routine the host entry point
// (gpudiff_render_value_from_blob) and kernels K21 / K22 (values.hip) share.
// Internal, not part of the ABI.  Plain C++: no HIP header, so a host program
// compiles it alone.
//
// The text is what the write path's encoder puts on the wire for the leaf
// (json.NewEncoder(w).Encode, restated by go_marshal.cpp and K10), rendered from
// the canonical value the blob stores: the literals, int64 digits, Go's
// shortest float64 form, and a string as '"' + HTML-safe escaping + '"'.
//
// A string's bytes are read through an accessor -- bytes 0..7 from vals, bytes
// 8.. from the arena tail -- so an escape that straddles the head / tail
// boundary (U+2028 starting at decoded byte 6 or 7) is seen whole.
//
// Nothing here trusts the blob: a segment, leaf index, arena offset or tail
// outside the bytes given, an arena prefix beyond the row's arena size, a len
// that does not fit the tag all end as "unresolved".  The write pass never
// stores outside dst[0, len).
//
// The float digits are the caller's: fmt(bits, out) returns the length of Go's
// text of the float64 `bits` and writes it when out != nullptr (the device
// passes go_float_put, the host the formatter of go_marshal.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gpudiff_format.h"

namespace gd {

constexpr uint64_t kValUnresolved = ~0ull;
constexpr uint32_t kValNoLeaf = 0xFFFFFFFFu;

// one region's segment of a blob; ok = false when it does not lie inside the bytes given
struct ValSeg {
    const uint8_t* vals;   // [l] u64 (byte pointers: the host's copy of a blob sits wherever the caller put it)
    const uint8_t* keys;   // [l] u32
    const uint8_t* metas;  // [l] u32
    const uint8_t* arena;  // [ar] bytes
    uint32_t l, ar;
    bool ok;
};

// in HBM a blob starts on a 128-B line, so its words are aligned; the host's copy sits wherever the caller put it
GPUDIFF_HD inline uint32_t val_ld32(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *(const uint32_t*)p;
#else
    uint32_t x;
    __builtin_memcpy(&x, p, 4);
    return x;
#endif
}
GPUDIFF_HD inline uint64_t val_ld64(const uint8_t* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *(const uint64_t*)p;
#else
    uint64_t x;
    __builtin_memcpy(&x, p, 8);
    return x;
#endif
}

// the spec (status = false) or status segment of the blob at `blob` with `room` readable bytes
GPUDIFF_HD inline ValSeg val_seg(const uint8_t* blob, uint64_t room, uint32_t spec_l, uint32_t spec_ar, uint32_t stat_l,
                                 uint32_t stat_ar, bool status) {
    ValSeg s;
    const uint64_t base = status ? gpudiff_seg_bytes(spec_l, spec_ar) : 0;
    s.l = status ? stat_l : spec_l;
    s.ar = status ? stat_ar : spec_ar;
    const uint64_t bytes = gpudiff_seg_bytes(s.l, s.ar);
    s.ok = base <= room && bytes <= room - base;
    s.vals = blob + (s.ok ? base : 0);
    s.keys = s.vals + 8ull * s.l;
    s.metas = s.keys + 4ull * s.l;
    s.arena = s.metas + 4ull * s.l;
    if (!s.ok) s.l = s.ar = 0;
    return s;
}

GPUDIFF_HD inline uint32_t val_meta(const ValSeg& s, uint32_t i) { return val_ld32(s.metas + 4ull * i); }

// index of the leaf whose key is h, or kValNoLeaf
GPUDIFF_HD inline uint32_t val_find(const ValSeg& s, uint64_t h) {
    if (h > 0xFFFFFFFFull) return kValNoLeaf;
    uint32_t lo = 0, hi = s.l;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (val_ld32(s.keys + 4ull * mid) < (uint32_t)h) lo = mid + 1;
        else hi = mid;
    }
    return (lo < s.l && val_ld32(s.keys + 4ull * lo) == (uint32_t)h) ? lo : kValNoLeaf;
}

// arena offset of leaf idx's tail: the arena bytes of the leaves before it (one pass from 0: the host's way;
// the kernels derive a pair's offsets in one forward sweep instead)
GPUDIFF_HD inline uint64_t val_arena_prefix(const ValSeg& s, uint32_t idx) {
    uint64_t a = 0;
    for (uint32_t i = 0; i < idx && i < s.l; i++) a += gpudiff_meta_arena(val_meta(s, i));
    return a;
}

// one leaf, checked: its meta fits its tag and its tail lies inside the arena
struct ValLeaf {
    uint64_t head;        // vals[idx]
    const uint8_t* tail;  // the arena tail of a long string
    uint32_t tag, len;
    bool ok;
};

GPUDIFF_HD inline ValLeaf val_leaf(const ValSeg& s, uint32_t idx, uint64_t aoff) {
    ValLeaf v;
    v.head = 0;
    v.tail = s.arena;
    v.tag = v.len = 0;
    v.ok = false;
    if (!s.ok || idx >= s.l) return v;
    const uint32_t m = val_meta(s, idx);
    v.tag = gpudiff_meta_tag(m);
    v.len = gpudiff_meta_len(m);
    v.head = val_ld64(s.vals + 8ull * idx);
    if (v.tag == GPUDIFF_TAG_INT || v.tag == GPUDIFF_TAG_FLOAT) v.ok = v.len == 8;
    else if (v.tag == GPUDIFF_TAG_STR)
        v.ok = !gpudiff_meta_is_long(m) || (aoff <= s.ar && gpudiff_meta_arena(m) <= s.ar - aoff);
    else v.ok = v.len == 0;
    if (v.ok && gpudiff_meta_is_long(m)) v.tail = s.arena + aoff;
    return v;
}

// decoded byte i of a string leaf
GPUDIFF_HD inline uint32_t val_byte(const ValLeaf& v, uint32_t i) {
    return i < GPUDIFF_INLINE_MAX ? (uint32_t)((v.head >> (8u * i)) & 0xFFu) : (uint32_t)v.tail[i - GPUDIFF_INLINE_MAX];
}

// output bytes of decoded byte i of a string of n bytes (1, 2 or 6; the three bytes of U+2028 / U+2029 give
// 6, 0, 0): Go 1.16 encodeState.string(s, escapeHTML=true) over valid UTF-8, byte by byte
GPUDIFF_HD inline uint32_t val_esc_unit(const ValLeaf& v, uint32_t n, uint32_t i) {
    const uint32_t c = val_byte(v, i);
    if (c < 0x80u) {
        if (c == '"' || c == '\\' || c == '\n' || c == '\r' || c == '\t') return 2;
        return (c < 0x20u || c == '<' || c == '>' || c == '&') ? 6u : 1u;
    }
    if (c == 0xE2u) {
        if (!(i + 2 < n && val_byte(v, i + 1) == 0x80u)) return 1u;
        const uint32_t t = val_byte(v, i + 2);
        return (t == 0xA8u || t == 0xA9u) ? 6u : 1u;
    }
    if (c == 0x80u) {
        if (!(i >= 1 && i + 1 < n && val_byte(v, i - 1) == 0xE2u)) return 1u;
        const uint32_t t = val_byte(v, i + 1);
        return (t == 0xA8u || t == 0xA9u) ? 0u : 1u;
    }
    if (c == 0xA8u || c == 0xA9u)
        return (i >= 2 && val_byte(v, i - 1) == 0x80u && val_byte(v, i - 2) == 0xE2u) ? 0u : 1u;
    return 1u;
}

// the u output bytes of decoded byte i (u = val_esc_unit's answer) at q
GPUDIFF_HD inline void val_esc_emit(const ValLeaf& v, uint32_t i, uint32_t u, uint8_t* q) {
    const uint32_t c = val_byte(v, i);
    if (u == 1) {
        q[0] = (uint8_t)c;
    } else if (u == 2) {
        q[0] = '\\';
        q[1] = c == '\n' ? 'n' : c == '\r' ? 'r' : c == '\t' ? 't' : (uint8_t)c;
    } else if (u == 6) {
        q[0] = '\\';
        q[1] = 'u';
        if (c == 0xE2u) {
            q[2] = '2';
            q[3] = '0';
            q[4] = '2';
            q[5] = val_byte(v, i + 2) == 0xA8u ? '8' : '9';
        } else {
            const uint32_t hi = c >> 4, lo = c & 15u;
            q[2] = '0';
            q[3] = '0';
            q[4] = (uint8_t)('0' + hi);  // c < 0x40 here: one decimal digit
            q[5] = (uint8_t)(lo < 10u ? '0' + lo : 'a' + (lo - 10u));
        }
    }
}

GPUDIFF_HD inline uint32_t val_i64_len(uint64_t bits) {
    const bool neg = (bits >> 63) != 0;
    uint64_t u = neg ? 0ull - bits : bits;
    uint32_t n = neg ? 2u : 1u;
    while (u >= 10u) {
        u /= 10u;
        n++;
    }
    return n;
}
GPUDIFF_HD inline void val_i64_put(uint8_t* o, uint64_t bits, uint32_t n) {
    const bool neg = (bits >> 63) != 0;
    uint64_t u = neg ? 0ull - bits : bits;
    for (uint32_t k = n; k-- > (neg ? 1u : 0u);) {
        o[k] = (uint8_t)('0' + u % 10u);
        u /= 10u;
    }
    if (neg) o[0] = '-';
}

GPUDIFF_HD inline const char* val_literal(uint32_t tag) {
    return tag == GPUDIFF_TAG_NULL ? "null" : tag == GPUDIFF_TAG_FALSE ? "false" : tag == GPUDIFF_TAG_TRUE ? "true"
         : tag == GPUDIFF_TAG_EOBJ ? "{}" : "[]";
}
GPUDIFF_HD inline uint32_t val_literal_len(uint32_t tag) {
    return tag == GPUDIFF_TAG_NULL || tag == GPUDIFF_TAG_TRUE ? 4u : tag == GPUDIFF_TAG_FALSE ? 5u : 2u;
}

// length of the leaf's text (never 0), or kValUnresolved; strings are walked byte by byte
template <class FloatFmt>
GPUDIFF_HD inline uint64_t val_text_len(const ValLeaf& v, FloatFmt fmt) {
    if (!v.ok) return kValUnresolved;
    if (v.tag == GPUDIFF_TAG_INT) return val_i64_len(v.head);
    if (v.tag == GPUDIFF_TAG_FLOAT) return fmt(v.head, (uint8_t*)nullptr);
    if (v.tag != GPUDIFF_TAG_STR) return val_literal_len(v.tag);
    uint64_t n = 2;
    for (uint32_t i = 0; i < v.len; i++) n += val_esc_unit(v, v.len, i);
    return n;
}

// writes the text into dst[0, len), len = val_text_len's answer for the same leaf.  Whatever len is, nothing
// outside dst[0, len) is touched; false (dst's contents undefined) when the text's length is not len
template <class FloatFmt>
GPUDIFF_HD inline bool val_text_write(const ValLeaf& v, uint8_t* dst, uint64_t len, FloatFmt fmt) {
    if (!v.ok) return false;
    if (v.tag == GPUDIFF_TAG_INT) {
        const uint32_t n = val_i64_len(v.head);
        if (n != len) return false;
        val_i64_put(dst, v.head, n);
        return true;
    }
    if (v.tag == GPUDIFF_TAG_FLOAT) {
        if (fmt(v.head, (uint8_t*)nullptr) != len) return false;
        return fmt(v.head, dst) == len;
    }
    if (v.tag != GPUDIFF_TAG_STR) {
        const uint32_t n = val_literal_len(v.tag);
        if (n != len) return false;
        const char* s = val_literal(v.tag);
        for (uint32_t q = 0; q < n; q++) dst[q] = (uint8_t)s[q];
        return true;
    }
    if (len < 2) return false;
    uint64_t cur = 1;
    dst[0] = '"';
    for (uint32_t i = 0; i < v.len; i++) {
        const uint32_t u = val_esc_unit(v, v.len, i);
        if (cur + u > len - 1) return false;
        val_esc_emit(v, i, u, dst + cur);
        cur += u;
    }
    if (cur != len - 1) return false;
    dst[cur] = '"';
    return true;
}

}  // namespace gd
