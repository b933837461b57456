// The Update body's host path under AddressSanitizer / UndefinedBehaviorSanitizer: a stand-alone program (its own
// main, nothing loaded into an interpreter, no GPU work) over gpudiff_upsert_body_host_rv,
// gpudiff_update_body_host and gpudiff_splice_resource_version: the known answers of tests/test_update_body.py,
// exact-size and short output buffers, and descriptors that do not fit the body.
//
// The host marshaller is go_marshal.cpp over json.cpp and needs nothing else of the library
// (tests/test_go_marshal_sanitize.py builds and runs this program so):
//
//   S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   g++ -O1 -g -std=c++17 -Wall -Werror $S -Iinclude -o /tmp/ubs tools/update_body_sanitize.cpp kcp_amd/csrc/go_marshal.cpp kcp_amd/csrc/json.cpp
//   /tmp/ubs
//
// Exit status 0 and "ok" = every answer matched and the sanitizers saw nothing.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "gpudiff.h"

namespace {

int g_fail = 0;

void expect(bool ok, const char* what, size_t k) {
    if (ok) return;
    fprintf(stderr, "FAIL case %zu: %s\n", k, what);
    g_fail++;
}

struct Case {
    std::string doc;
    uint32_t mode;
    std::string rv, body, update;
    uint32_t off, form;
};

const uint32_t I = GPUDIFF_RV_INSERT, L = GPUDIFF_RV_LEAD, T = GPUDIFF_RV_TRAIL, W = GPUDIFF_RV_WRAP;

// each entry point into a heap buffer of exactly the size it asked for (so an overrun of one byte is seen)
template <class F>
bool sized(F&& call, std::string* out, int* rc_out) {
    size_t n = 0;
    int rc = call(nullptr, 0, &n);
    *rc_out = rc;
    if (rc != GPUDIFF_E_CAPACITY && !(rc == GPUDIFF_OK && n == 0)) return false;
    std::vector<uint8_t> buf(n);
    size_t m = 0;
    rc = call(buf.data(), n, &m);
    *rc_out = rc;
    if (rc != GPUDIFF_OK || m != n) return false;
    out->assign((const char*)buf.data(), n);
    if (n > 1) {  // one byte short: GPUDIFF_E_CAPACITY with the length, nothing written past the buffer
        std::vector<uint8_t> small(n - 1);
        size_t q = 0;
        if (call(small.data(), n - 1, &q) != GPUDIFF_E_CAPACITY || q != n) return false;
    }
    return true;
}

}  // namespace

int main() {
    const std::string own = "\"labels\":{\"kcp.dev/owned-by\":\"own\"}";
    const std::string ref = "\"ownerReferences\":[{\"name\":\"own\"}]";
    const std::vector<Case> cases = {
        {"{\"metadata\":{\"name\":\"a\",\"uid\":\"u\",\"resourceVersion\":\"1\"},\"kind\":\"K\"}", 0, "42",
         "{\"kind\":\"K\",\"metadata\":{\"name\":\"a\"}}\n",
         "{\"kind\":\"K\",\"metadata\":{\"name\":\"a\",\"resourceVersion\":\"42\"}}\n", 34, I | L},
        {"{\"metadata\":{\"uid\":\"u\"}}", 0, "42", "{\"metadata\":{}}\n",
         "{\"metadata\":{\"resourceVersion\":\"42\"}}\n", 13, I},
        {"{\"b\":1,\"a\":2}", 0, "42", "{\"a\":2,\"b\":1}\n",
         "{\"a\":2,\"b\":1,\"metadata\":{\"resourceVersion\":\"42\"}}\n", 12, I | L | W},
        {"{}", 1, "42", "{}\n", "{\"metadata\":{\"resourceVersion\":\"42\"}}\n", 1, I | W},
        {"{\"spec\":{}}", 0, "42", "{\"spec\":{}}\n", "{\"metadata\":{\"resourceVersion\":\"42\"},\"spec\":{}}\n", 1,
         I | T | W},
        {"{\"spec\":{},\"kind\":\"K\"}", 0, "42", "{\"kind\":\"K\",\"spec\":{}}\n",
         "{\"kind\":\"K\",\"metadata\":{\"resourceVersion\":\"42\"},\"spec\":{}}\n", 11, I | L | W},
        {"{\"metadata\":null,\"x\":1}", 0, "42", "{\"metadata\":null,\"x\":1}\n", "{\"metadata\":null,\"x\":1}\n", 0, 0},
        {"{\"metadata\":\"s\"}", 1, "42", "{\"metadata\":\"s\"}\n", "{\"metadata\":\"s\"}\n", 0, 0},
        {"{\"metadata\":{\"selfLink\":\"s\",\"resourceVersion\":\"1\",\"name\":\"n\"}}", 1, "42",
         "{\"metadata\":{\"name\":\"n\",\"selfLink\":\"s\"}}\n",
         "{\"metadata\":{\"name\":\"n\",\"resourceVersion\":\"42\",\"selfLink\":\"s\"}}\n", 23, I | L},
        {"{\"metadata\":{\"resourceVersion\":\"1\",\"uid\":\"u\",\"zz\":1}}", 0, "42", "{\"metadata\":{\"zz\":1}}\n",
         "{\"metadata\":{\"resourceVersion\":\"42\",\"zz\":1}}\n", 13, I | T},
        {"{\"metadata\":{" + own + "," + ref + ",\"resourceVersion\":\"1\"}}", 0, "42",
         "{\"metadata\":{" + own + "}}\n", "{\"metadata\":{" + own + ",\"resourceVersion\":\"42\"}}\n",
         (uint32_t)(13 + own.size()), I | L},
        {"{\"metadata\":{\"ownerReferences\":[],\"resourceVersion\":\"1\"}}", 0, "42", "{\"metadata\":{}}\n",
         "{\"metadata\":{\"resourceVersion\":\"42\"}}\n", 13, I},
        {"{\"spec\":{\"metadata\":{\"resourceVersion\":\"9\"}}}", 0, "42",
         "{\"spec\":{\"metadata\":{\"resourceVersion\":\"9\"}}}\n",
         "{\"metadata\":{\"resourceVersion\":\"42\"},\"spec\":{\"metadata\":{\"resourceVersion\":\"9\"}}}\n", 1, I | T | W},
        {"{\"metadata\":{\"name\":\"a\"}}", 0, "a<b&\"\\", "{\"metadata\":{\"name\":\"a\"}}\n",
         "{\"metadata\":{\"name\":\"a\",\"resourceVersion\":\"a\\u003cb\\u0026\\\"\\\\\"}}\n", 23, I | L},
        {"{\"metadata\":{\"name\":\"a\"}}", 0, "\xff", "{\"metadata\":{\"name\":\"a\"}}\n",
         "{\"metadata\":{\"name\":\"a\",\"resourceVersion\":\"\\ufffd\"}}\n", 23, I | L},
        // a truncated sequence at the very end of rv: the validity check must not read past it
        {"{\"metadata\":{\"name\":\"a\"}}", 0, "\xe2\x80", "{\"metadata\":{\"name\":\"a\"}}\n",
         "{\"metadata\":{\"name\":\"a\",\"resourceVersion\":\"\\ufffd\\ufffd\"}}\n", 23, I | L},
        {"{\"metadata\":{\"name\":\"a\",\"resourceVersion\":\"1\"}}", 1, "", "{\"metadata\":{\"name\":\"a\"}}\n",
         "{\"metadata\":{\"name\":\"a\"}}\n", 23, I | L},
    };
    for (size_t k = 0; k < cases.size(); k++) {
        const Case& c = cases[k];
        // heap copies of exactly the inputs' sizes: a read past a document or rv is seen
        const std::vector<uint8_t> doc(c.doc.begin(), c.doc.end()), rv(c.rv.begin(), c.rv.end());
        std::string body, update, spliced;
        uint32_t off = 99, form = 99;
        int rc = 0;
        expect(sized([&](uint8_t* o, size_t cap, size_t* n) {
                   return gpudiff_upsert_body_host_rv(doc.data(), doc.size(), c.mode, o, cap, n, &off, &form);
               }, &body, &rc), "upsert_body_host_rv", k);
        expect(body == c.body && off == c.off && form == c.form, "body / descriptor", k);
        expect(sized([&](uint8_t* o, size_t cap, size_t* n) {
                   return gpudiff_update_body_host(doc.data(), doc.size(), c.mode, rv.data(), rv.size(), o, cap, n);
               }, &update, &rc), "update_body_host", k);
        expect(update == c.update, "update body", k);
        const std::vector<uint8_t> b(body.begin(), body.end());
        expect(sized([&](uint8_t* o, size_t cap, size_t* n) {
                   return gpudiff_splice_resource_version(b.data(), b.size(), off, form, rv.data(), rv.size(), o, cap, n);
               }, &spliced, &rc), "splice", k);
        expect(spliced == c.update, "spliced body", k);
    }
    // descriptors that do not fit the body, unknown form bits, decode errors
    const std::string body = "{\"metadata\":{}}\n";
    const std::vector<uint8_t> b(body.begin(), body.end());
    uint8_t out[128];
    size_t n = 0;
    const uint32_t bad[][2] = {{(uint32_t)b.size(), I}, {(uint32_t)b.size() + 1, I}, {0, I}, {0xFFFFFFFFu, I | L},
                               {13, 0x10}, {13, I | 0x80}, {13, L}, {13, W | T}, {(uint32_t)b.size() + 1, 0},
                               {0x80000000u, I | W}};
    for (size_t k = 0; k < sizeof(bad) / sizeof(bad[0]); k++)
        expect(gpudiff_splice_resource_version(b.data(), b.size(), bad[k][0], bad[k][1], (const uint8_t*)"42", 2, out,
                                               sizeof(out), &n) == GPUDIFF_E_INVAL, "E_INVAL", 100 + k);
    expect(gpudiff_splice_resource_version(b.data(), b.size(), 13, I, (const uint8_t*)"42", 2, out, sizeof(out),
                                           nullptr) == GPUDIFF_E_INVAL, "null out_len", 120);
    expect(gpudiff_update_body_host((const uint8_t*)"[", 1, 0, (const uint8_t*)"1", 1, out, sizeof(out), &n) ==
               GPUDIFF_E_DECODE && n == 0, "decode error", 121);
    expect(gpudiff_update_body_host(nullptr, 0, 0, nullptr, 0, out, sizeof(out), &n) == GPUDIFF_E_DECODE, "empty", 122);
    if (g_fail) return 1;
    printf("ok: %zu known answers, %zu refused descriptors\n", cases.size(), sizeof(bad) / sizeof(bad[0]));
    return 0;
}
