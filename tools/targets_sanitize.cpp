// The request target's host path under AddressSanitizer / UndefinedBehaviorSanitizer: a stand-alone program (its own
// main, nothing loaded into an interpreter, no GPU work) over gpudiff_upsert_body_host_targets,
// gpudiff_target_decode, gpudiff_target_host and gpudiff_targets_namespaces: known answers of tests/test_targets.py,
// exact-size and short output buffers, spans that leave the body, malformed escapes -- and, given a corpus file, every
// document of it in both modes: the decoded spans must equal gpudiff_target_host's strings.
//
// The corpus file is the write path's test corpus (tests/upsert_cases.py: the KAT documents, fixture_docs(),
// boundary_docs() and synthetic_docs(), in that order), each document behind its length (u32, little-endian).
// tests/test_go_marshal_sanitize.py writes it.
//
// The host marshaller is go_marshal.cpp over json.cpp and needs nothing else of the library
// (tests/test_go_marshal_sanitize.py builds and runs this program so):
//
//   S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   g++ -O1 -g -std=c++17 -Wall -Werror $S -Iinclude -o /tmp/tgs tools/targets_sanitize.cpp kcp_amd/csrc/go_marshal.cpp kcp_amd/csrc/json.cpp
//   /tmp/tgs /tmp/corpus.bin
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

const uint32_t N = GPUDIFF_TGT_NAME, NE = GPUDIFF_TGT_NAME_ESC, S = GPUDIFF_TGT_NS, SE = GPUDIFF_TGT_NS_ESC;

struct Case {
    std::string doc;
    uint32_t mode;
    std::string body;
    uint32_t name_off, name_len, ns_off, ns_len, flags;
    std::string ns, name;
};

struct Desc {
    uint32_t off[2] = {99, 99}, len[2] = {99, 99}, flags = 99;
};

// the body into a heap buffer of exactly its size (an overrun of one byte is seen), and once into one a byte short
bool body_of(const std::vector<uint8_t>& doc, uint32_t mode, std::string* body, Desc* d, int* rc_out) {
    size_t n = 0;
    int rc = gpudiff_upsert_body_host_targets(doc.data(), doc.size(), mode, nullptr, 0, &n, d->off, d->len, &d->flags);
    *rc_out = rc;
    if (rc != GPUDIFF_E_CAPACITY) return false;
    std::vector<uint8_t> buf(n), small(n - 1);
    size_t m = 0, q = 0;
    Desc again;
    if (gpudiff_upsert_body_host_targets(doc.data(), doc.size(), mode, small.data(), n - 1, &q, again.off, again.len,
                                         &again.flags) != GPUDIFF_E_CAPACITY || q != n)
        return false;
    rc = gpudiff_upsert_body_host_targets(doc.data(), doc.size(), mode, buf.data(), n, &m, d->off, d->len, &d->flags);
    *rc_out = rc;
    if (rc != GPUDIFF_OK || m != n) return false;
    body->assign((const char*)buf.data(), n);
    return true;
}

// a span decoded into a heap buffer of exactly the decoded size
bool decoded(const std::vector<uint8_t>& body, uint32_t off, uint32_t len, std::string* out) {
    size_t n = 0;
    const int rc = gpudiff_target_decode(body.data(), body.size(), off, len, nullptr, 0, &n);
    if (rc != (n ? GPUDIFF_E_CAPACITY : GPUDIFF_OK)) return false;
    std::vector<uint8_t> buf(n);
    size_t m = 0;
    if (gpudiff_target_decode(body.data(), body.size(), off, len, buf.data(), n, &m) != GPUDIFF_OK || m != n)
        return false;
    if (n > 1) {
        std::vector<uint8_t> small(n - 1);
        size_t q = 0;
        if (gpudiff_target_decode(body.data(), body.size(), off, len, small.data(), n - 1, &q) != GPUDIFF_E_CAPACITY ||
            q != n)
            return false;
    }
    out->assign((const char*)buf.data(), n);
    return true;
}

// gpudiff_target_host into heap buffers of exactly the values' sizes
bool host_of(const std::vector<uint8_t>& doc, std::string* ns, std::string* name, int* rc_out) {
    size_t nn = 0, sn = 0;
    int rc = gpudiff_target_host(doc.data(), doc.size(), nullptr, 0, &nn, nullptr, 0, &sn);
    *rc_out = rc;
    if (rc != GPUDIFF_OK && rc != GPUDIFF_E_CAPACITY) return false;
    std::vector<uint8_t> nb(nn), sb(sn);
    rc = gpudiff_target_host(doc.data(), doc.size(), nb.data(), nn, &nn, sb.data(), sn, &sn);
    *rc_out = rc;
    if (rc != GPUDIFF_OK) return false;
    name->assign((const char*)nb.data(), nn);
    ns->assign((const char*)sb.data(), sn);
    return true;
}

// one document: body + descriptor, both spans decoded, against the direct decode; *ns_key = the rendered namespace
bool cross_check(const std::vector<uint8_t>& doc, uint32_t mode, std::string* body, Desc* d, std::string* ns,
                 std::string* name, bool* decode_error) {
    int rc = 0, hrc = 0;
    *decode_error = false;
    if (!body_of(doc, mode, body, d, &rc)) {
        std::string a, b;
        *decode_error = rc == GPUDIFF_E_DECODE && !host_of(doc, &a, &b, &hrc) && hrc == GPUDIFF_E_DECODE &&
                        d->flags == 0 && d->off[0] == 0 && d->off[1] == 0 && d->len[0] == 0 && d->len[1] == 0;
        return false;
    }
    const std::vector<uint8_t> b(body->begin(), body->end());
    std::string hns, hname;
    if (!decoded(b, d->off[0], d->len[0], name) || !decoded(b, d->off[1], d->len[1], ns)) return false;
    if (!host_of(doc, &hns, &hname, &hrc)) return false;
    for (int k = 0; k < 2; k++) {  // canonical form
        const uint32_t present = d->flags >> (2 * k) & N, esc = d->flags >> (2 * k) & NE;
        if (!present && (d->off[k] || d->len[k] || esc)) return false;
        if (present && (d->off[k] == 0 || (*body)[d->off[k] - 1] != '"' || (*body)[d->off[k] + d->len[k]] != '"'))
            return false;
        if ((esc != 0) != (memchr(body->data() + d->off[k], '\\', d->len[k]) != nullptr)) return false;
    }
    return hns == *ns && hname == *name;
}

}  // namespace

int main(int argc, char** argv) {
    const std::vector<Case> cases = {
        {"{\"metadata\":{\"name\":\"a\",\"uid\":\"u\",\"resourceVersion\":\"1\"},\"kind\":\"K\"}", 0,
         "{\"kind\":\"K\",\"metadata\":{\"name\":\"a\"}}\n", 32, 1, 0, 0, N, "", "a"},
        {"{\"metadata\":{\"namespace\":\"ns1\",\"name\":\"n1\"}}", 1,
         "{\"metadata\":{\"name\":\"n1\",\"namespace\":\"ns1\"}}\n", 21, 2, 38, 3, N | S, "ns1", "n1"},
        {"{\"metadata\":{\"name\":\"\",\"namespace\":\"\"}}", 0, "{\"metadata\":{\"name\":\"\",\"namespace\":\"\"}}\n", 21, 0,
         36, 0, N | S, "", ""},
        {"{\"metadata\":{\"name\":\"a<b\",\"namespace\":\"x\\\"y\\\\z\xe2\x80\xa8\"}}", 1,
         "{\"metadata\":{\"name\":\"a\\u003cb\",\"namespace\":\"x\\\"y\\\\z\\u2028\"}}\n", 21, 8, 44, 13, N | NE | S | SE,
         "x\"y\\z\xe2\x80\xa8", "a<b"},
        {"{\"metadata\":{\"name\":\"\\u0061b\",\"namespace\":\"caf\xc3\xa9\"}}", 0,
         "{\"metadata\":{\"name\":\"ab\",\"namespace\":\"caf\xc3\xa9\"}}\n", 21, 2, 38, 5, N | S, "caf\xc3\xa9", "ab"},
        {"{\"metadata\":null,\"x\":1}", 0, "{\"metadata\":null,\"x\":1}\n", 0, 0, 0, 0, 0, "", ""},
        {"{\"metadata\":{\"name\":5,\"namespace\":null}}", 0, "{\"metadata\":{\"name\":5,\"namespace\":null}}\n", 0, 0, 0,
         0, 0, "", ""},
        {"{\"metadata\":{\"name\":\"a\",\"name\":\"b\"}}", 0, "{\"metadata\":{\"name\":\"b\"}}\n", 21, 1, 0, 0, N, "", "b"},
        {"{\"metadata\":{\"name\":\"a\"},\"metadata\":{\"namespace\":\"q\"}}", 1, "{\"metadata\":{\"namespace\":\"q\"}}\n",
         0, 0, 26, 1, S, "q", ""},
        {"{\"metadata\":{\"n\\u0061me\":\"x\",\"namesp\\u0061ce\":\"y\"}}", 0,
         "{\"metadata\":{\"name\":\"x\",\"namespace\":\"y\"}}\n", 21, 1, 37, 1, N | S, "y", "x"},
        {"{\"name\":\"r\",\"spec\":{\"metadata\":{\"name\":\"s\"}},\"metadata\":{\"ownerReferences\":[{\"name\":\"o\"}]}}", 0,
         "{\"metadata\":{\"ownerReferences\":[{\"apiVersion\":\"\",\"kind\":\"\",\"name\":\"o\",\"uid\":\"\"}]},\"name\":\"r\","
         "\"spec\":{\"metadata\":{\"name\":\"s\"}}}\n", 0, 0, 0, 0, 0, "", ""},
    };
    std::vector<std::string> bodies;
    std::vector<Desc> descs;
    for (size_t k = 0; k < cases.size(); k++) {
        const Case& c = cases[k];
        // a heap copy of exactly the input's size: a read past the document is seen
        const std::vector<uint8_t> doc(c.doc.begin(), c.doc.end());
        std::string body, ns, name;
        Desc d;
        bool derr = false;
        expect(cross_check(doc, c.mode, &body, &d, &ns, &name, &derr), "body / spans / direct decode", k);
        expect(body == c.body, "body", k);
        expect(d.off[0] == c.name_off && d.len[0] == c.name_len && d.off[1] == c.ns_off && d.len[1] == c.ns_len &&
                   d.flags == c.flags, "descriptor", k);
        expect(ns == c.ns && name == c.name, "strings", k);
        bodies.push_back(body);
        descs.push_back(d);
    }
    // gpudiff_targets_namespaces over the known answers' bodies, a no-op write and an undecodable one among them
    {
        bodies.insert(bodies.begin() + 2, std::string());
        descs.insert(descs.begin() + 2, Desc{{0, 0}, {0, 0}, 0});
        const size_t n = bodies.size();
        std::vector<uint64_t> offsets(n + 1, 0);
        std::vector<uint8_t> bytes;
        std::vector<int32_t> status(n, 0);
        std::vector<uint32_t> off(2 * n), len(2 * n);
        std::vector<uint8_t> flags(n);
        for (size_t w = 0; w < n; w++) {
            bytes.insert(bytes.end(), bodies[w].begin(), bodies[w].end());
            offsets[w + 1] = bytes.size();
            for (int k = 0; k < 2; k++) {
                off[2 * w + k] = descs[w].off[k];
                len[2 * w + k] = descs[w].len[k];
            }
            flags[w] = (uint8_t)descs[w].flags;
        }
        status[5] = GPUDIFF_E_DECODE;  // as if Go had not decoded it: not grouped, whatever its bytes
        gpudiff_bodies b{};
        b.n = n;
        b.offsets = offsets.data();
        b.bytes = bytes.data();
        b.status = status.data();
        gpudiff_targets t{};
        t.n = n;
        t.off = off.data();
        t.len = len.data();
        t.flags = flags.data();
        std::vector<uint32_t> group_of(n, 7), first(n, 7), clusters(n);
        std::vector<uint8_t> skip(n, 0);
        for (size_t w = 0; w < n; w++) clusters[w] = (uint32_t)(w % 2);
        skip[0] = 1;
        size_t ng = 99;
        expect(gpudiff_targets_namespaces(&b, &t, nullptr, nullptr, group_of.data(), first.data(), &ng) == GPUDIFF_OK,
               "namespaces", 200);
        // namespaces in order: "" (0), ns1 (1), [no body], "" , x"y\z..., [decode error], "", "", "", q, y, ""
        const uint32_t X = 0xFFFFFFFFu;
        const std::vector<uint32_t> want = {0, 1, X, 0, 2, X, 0, 0, 0, 3, 4, 0};
        expect(ng == 5 && group_of == want && first[0] == 0 && first[1] == 1 && first[2] == 4 && first[3] == 9 &&
                   first[4] == 10, "namespaces: groups", 201);
        expect(gpudiff_targets_namespaces(&b, &t, clusters.data(), skip.data(), group_of.data(), first.data(), &ng) ==
                   GPUDIFF_OK && group_of[0] == X && group_of[3] == 1 && group_of[1] == 0 && ng == 6,
               "namespaces: clusters and skip", 202);
        len[2 * 1 + 1] = (uint32_t)bodies[1].size();  // a span that leaves its body
        expect(gpudiff_targets_namespaces(&b, &t, nullptr, nullptr, group_of.data(), first.data(), &ng) ==
                   GPUDIFF_E_INVAL, "namespaces: E_INVAL", 203);
        t.n = n - 1;
        expect(gpudiff_targets_namespaces(&b, &t, nullptr, nullptr, group_of.data(), first.data(), &ng) ==
                   GPUDIFF_E_INVAL, "namespaces: other bodies' targets", 204);
    }
    // spans that leave the body, malformed escapes
    {
        const std::string body = "{\"a\":\"xy\"}\n";
        const std::vector<uint8_t> b(body.begin(), body.end());
        uint8_t out[64];
        size_t n = 0;
        const uint32_t bad[][2] = {{(uint32_t)b.size() + 1, 0}, {(uint32_t)b.size(), 1}, {6, (uint32_t)b.size()},
                                   {0xFFFFFFFFu, 2}, {2, 0xFFFFFFFFu}};
        for (size_t k = 0; k < sizeof(bad) / sizeof(bad[0]); k++)
            expect(gpudiff_target_decode(b.data(), b.size(), bad[k][0], bad[k][1], out, sizeof(out), &n) ==
                       GPUDIFF_E_INVAL, "span: E_INVAL", 300 + k);
        const char* mal[] = {"\\", "ab\\", "\\x", "\\/", "\\u12", "\\u12G4", "\\u", "a\\u00e", "\\ud83d\\ude0"};
        for (size_t k = 0; k < sizeof(mal) / sizeof(mal[0]); k++) {
            const std::vector<uint8_t> m(mal[k], mal[k] + strlen(mal[k]));  // exactly sized: no read past the span
            expect(gpudiff_target_decode(m.data(), m.size(), 0, (uint32_t)m.size(), out, sizeof(out), &n) ==
                       GPUDIFF_E_INVAL, "escape: E_INVAL", 320 + k);
        }
        const std::string every = "\\\"\\\\\\n\\r\\t\\b\\f\\u00e9\\u2028\\ud83d\\ude00\\ud800x\\ud800";
        const std::vector<uint8_t> e(every.begin(), every.end());
        std::string dec;
        expect(decoded(e, 0, (uint32_t)e.size(), &dec) &&
                   dec == "\"\\\n\r\t\b\f\xc3\xa9\xe2\x80\xa8\xf0\x9f\x98\x80\xef\xbf\xbdx\xef\xbf\xbd", "every escape", 340);
        expect(gpudiff_target_decode(b.data(), b.size(), 6, 2, out, sizeof(out), nullptr) == GPUDIFF_E_INVAL,
               "null out_len", 341);
        expect(gpudiff_target_host((const uint8_t*)"[", 1, out, 8, &n, out + 8, 8, &n) == GPUDIFF_E_DECODE, "decode", 342);
        expect(gpudiff_target_host(nullptr, 0, out, 8, &n, out + 8, 8, &n) == GPUDIFF_E_DECODE, "empty", 343);
    }
    // the corpus, both modes
    size_t n_docs = 0, n_err = 0;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        uint8_t lb[4];
        while (fread(lb, 1, 4, f) == 4) {
            const uint32_t len = lb[0] | lb[1] << 8 | lb[2] << 16 | (uint32_t)lb[3] << 24;
            std::vector<uint8_t> doc(len);
            if (len && fread(doc.data(), 1, len, f) != len) {
                fprintf(stderr, "short corpus file\n");
                return 2;
            }
            for (uint32_t mode = 0; mode < 2; mode++) {
                std::string body, ns, name;
                Desc d;
                bool derr = false;
                const bool ok = cross_check(doc, mode, &body, &d, &ns, &name, &derr);
                expect(ok || derr, "corpus document", 1000 + n_docs);
                n_err += derr ? 1 : 0;
            }
            n_docs++;
        }
        fclose(f);
    }
    if (g_fail) return 1;
    printf("ok: %zu known answers, %zu corpus documents (%zu decode errors over both modes)\n", cases.size(), n_docs, n_err);
    return 0;
}
