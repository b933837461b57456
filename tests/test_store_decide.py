"""PairEncoder::store_decide (kcp_amd/csrc/encoder.cpp): the one ladder both object stores take an event's old side
from -- resident blob at seed 0, pair re-encoded from old_json, resident blob at the slot's seed, first sighting
against {}, else conservative with store_seed.  One case per rung plus the store_seed fallback, on the host encoder
alone: 32-bit path hashes where nothing collides, 8-bit ones for forced collisions inside an object, 16-bit ones
for two paths that share a hash across the old and the new version (the path tables disagree).  The expected seeds
come from the encoder's primitives called on their own, never from store_decide."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "encoder.h"
#include <cstdio>
#include <cstdlib>
#include <string>
using namespace gd;

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s failed\n", __LINE__, #x); std::exit(1); } } while (0)

struct Fix {
    PairEncoder enc;
    Arena ao, an;
    FlatObject fo, fn;
    explicit Fix(uint32_t bits) : enc(EncodeConfig{bits}) {}
};
struct Tab {  // the slot's resident table, as the stores hand it over: counted, and able to fail
    const PathTable* t = nullptr;
    int rc = 0;
    int calls = 0;
    static int get(void* ctx, const PathTable** out) {
        Tab* t = (Tab*)ctx;
        t->calls++;
        *out = t->t;
        return t->rc;
    }
};
static StoreDecision decide(Fix& f, bool live, uint32_t seed, Tab& tab, const std::string* old_json,
                            const std::string& new_json) {
    tab.calls = 0;
    return f.enc.store_decide(live, seed, Tab::get, &tab, old_json ? (const uint8_t*)old_json->data() : nullptr,
                              old_json ? old_json->size() : 0, (const uint8_t*)new_json.data(), new_json.size(), f.ao,
                              f.an, f.fo, f.fn);
}
static void counters(const StoreDecision& d, uint32_t old_encoded, uint32_t reseeded, uint32_t unresolved) {
    CHECK(d.rc == 0);
    CHECK(d.old_encoded == old_encoded && d.reseeded == reseeded && d.unresolved == unresolved);
}
// `json` flattened and hashed under `seed` by a second encoder: its table, and whether hash_single took it
static bool table_of(uint32_t bits, const std::string& json, uint32_t seed, PathTable* out) {
    Fix g(bits);
    CHECK(g.enc.flatten_json((const uint8_t*)json.data(), json.size(), g.an, g.fn));
    const bool ok = g.enc.hash_single(g.fn, seed);
    *out = g.fn.tab;
    return ok;
}
static bool same_tab(const PathTable& a, const PathTable& b) { return a.n == b.n && a.data == b.data; }

static void rungs_32_bits() {
    Fix f(32);
    const std::string n1 = R"({"metadata":{"name":"x","labels":{"a":"b"}},"spec":{"replicas":1,"sel":{"k":"v"}},"status":{"ready":0}})";
    const std::string n2 = R"({"metadata":{"name":"x","labels":{"a":"b"}},"spec":{"replicas":2,"sel":{"k":"v"},"extra":[1,2]},"status":{"ready":1}})";
    const std::string bad = R"({"spec":)";
    Tab tab;
    PathTable none;
    none.n = GPUDIFF_TAB_NONE;

    // first sighting without an old object
    StoreDecision d = decide(f, false, 0, tab, nullptr, n1);
    CHECK(d.rung == StoreRung::kFirstSighting && d.seed == 0 && d.store_ok && tab.calls == 0);
    counters(d, 0, 0, 0);
    PathTable t1 = f.fn.tab, want;
    CHECK(t1.n != GPUDIFF_TAB_NONE && t1.n > 0);
    CHECK(table_of(32, n1, 0, &want) && same_tab(t1, want));

    // resident at seed 0 (old_json, when given, is not touched)
    tab.t = &t1;
    for (const std::string* old_json : {(const std::string*)nullptr, &n1}) {
        d = decide(f, true, 0, tab, old_json, n2);
        CHECK(d.rung == StoreRung::kResidentSeed0 && d.seed == 0 && d.store_ok && tab.calls == 1);
        counters(d, 0, 0, 0);
        CHECK(table_of(32, n2, 0, &want) && same_tab(f.fn.tab, want));
    }

    // re-encoded from old_json: a first sighting, and a slot re-seeded earlier (its table is not asked for)
    d = decide(f, false, 0, tab, &n1, n2);
    CHECK(d.rung == StoreRung::kReencodedOld && d.seed == 0 && d.store_ok && tab.calls == 0);
    counters(d, 1, 0, 0);
    CHECK(!f.fo.spec.empty() && !f.fn.spec.empty());
    d = decide(f, true, 5, tab, &n1, n2);
    CHECK(d.rung == StoreRung::kReencodedOld && d.seed == 0 && d.store_ok && tab.calls == 0);
    counters(d, 1, 1, 0);

    // resident at the slot's own seed
    PathTable t5;
    CHECK(table_of(32, n1, 5, &t5));
    tab.t = &t5;
    d = decide(f, true, 5, tab, nullptr, n2);
    CHECK(d.rung == StoreRung::kResidentSlotSeed && d.seed == 5 && d.store_ok && tab.calls == 1);
    counters(d, 0, 0, 0);
    CHECK(table_of(32, n2, 5, &want) && same_tab(f.fn.tab, want));  // fn is left hashed under the slot's seed

    // unresolved: a resident version that cannot vouch for its paths and no old object
    tab.t = &none;
    for (uint32_t seed : {0u, 5u}) {
        d = decide(f, true, seed, tab, nullptr, n2);
        CHECK(d.rung == StoreRung::kPairError && d.store_ok && d.seed == 0 && tab.calls == 1);
        counters(d, 0, 0, 1);
        CHECK(table_of(32, n2, 0, &want) && same_tab(f.fn.tab, want));  // store_seed: the smallest with a valid table
    }

    // an undecodable new object: nothing to store, nothing counted; an undecodable old one: the new one is stored
    d = decide(f, true, 0, tab, &n1, bad);
    CHECK(d.rung == StoreRung::kPairError && !d.store_ok && tab.calls == 0);
    counters(d, 0, 0, 0);
    d = decide(f, false, 0, tab, &bad, n2);
    CHECK(d.rung == StoreRung::kPairError && d.store_ok && d.seed == 0 && tab.calls == 0);
    counters(d, 0, 0, 0);

    // the resident table's error is passed through untouched, from either rung that reads it
    tab.t = &t1;
    tab.rc = 77;
    d = decide(f, true, 0, tab, &n1, n2);
    CHECK(d.rc == 77 && tab.calls == 1);
    tab.rc = -3;
    d = decide(f, true, 5, tab, nullptr, n2);
    CHECK(d.rc == -3 && tab.calls == 1);
}

static std::string wide(int i, int keys) {
    std::string s = "{\"spec\":{";
    for (int k = 0; k < keys; k++) s += (k ? ",\"k" : "\"k") + std::to_string(i) + "_" + std::to_string(k) + "\":0";
    return s + "}}";
}

static void forced_collisions_8_bits() {
    Fix f(8), g(8);
    Tab tab;
    // an object whose leaves collide under seed 0
    std::string coll;
    for (int i = 0; i < 1000 && coll.empty(); i++) {
        const std::string o = wide(i, 24);
        CHECK(g.enc.flatten_json((const uint8_t*)o.data(), o.size(), g.an, g.fn));
        if (!g.enc.hash_leaves(g.fn, 0)) coll = o;
    }
    CHECK(!coll.empty());
    uint32_t want = 0;
    CHECK(g.enc.flatten_json((const uint8_t*)coll.data(), coll.size(), g.an, g.fn) && g.enc.first_seed(g.fn, &want));
    CHECK(want != 0);
    StoreDecision d = decide(f, false, 0, tab, nullptr, coll);
    CHECK(d.rung == StoreRung::kFirstSighting && d.seed == want && d.store_ok && tab.calls == 0);
    counters(d, 0, 0, 0);

    // the same object arriving on a live slot at seed 0: re-seeded through old_json, to the pair's seed
    const std::string old_json = R"({"spec":{"a":1}})";
    PathTable told;
    CHECK(table_of(8, old_json, 0, &told));
    tab.t = &told;
    CHECK(g.enc.flatten_json((const uint8_t*)old_json.data(), old_json.size(), g.ao, g.fo) &&
          g.enc.flatten_json((const uint8_t*)coll.data(), coll.size(), g.an, g.fn) && g.enc.pair_seed(g.fo, g.fn, &want));
    CHECK(want != 0);
    d = decide(f, true, 0, tab, &old_json, coll);
    CHECK(d.rung == StoreRung::kReencodedOld && d.seed == want && d.store_ok && tab.calls == 1);
    counters(d, 1, 1, 0);
    CHECK(same_tab(f.fn.tab, g.fn.tab));

    // store_seed's fallback: more path-table nodes than 8-bit hashes, so no seed has a valid table, yet few enough
    // leaves that some seed keeps them apart: stored under first_seed's, without a table
    std::string deep = "{\"spec\":{";
    for (int c = 0; c < 20; c++) {
        deep += (c ? ",\"c" : "\"c") + std::to_string(c) + "\":";
        for (int l = 0; l < 13; l++) deep += "{\"d" + std::to_string(c) + "_" + std::to_string(l) + "\":";
        deep += "0" + std::string(13, '}');
    }
    deep += "}}";
    for (uint32_t s = 0; s <= 255; s++) {
        CHECK(g.enc.flatten_json((const uint8_t*)deep.data(), deep.size(), g.an, g.fn));
        CHECK(!g.enc.hash_single(g.fn, s));
    }
    CHECK(g.enc.flatten_json((const uint8_t*)deep.data(), deep.size(), g.an, g.fn) && g.enc.first_seed(g.fn, &want));
    d = decide(f, true, 0, tab, nullptr, deep);
    CHECK(d.rung == StoreRung::kPairError && d.store_ok && d.seed == want && tab.calls == 1);
    counters(d, 0, 0, 1);
    CHECK(f.fn.tab.n == GPUDIFF_TAB_NONE);

    // more leaves than hashes: no seed at all, the slot is emptied
    const std::string full = wide(0, 300);
    d = decide(f, false, 0, tab, nullptr, full);
    CHECK(d.rung == StoreRung::kPairError && !d.store_ok && tab.calls == 0);
    counters(d, 0, 0, 0);
}

static void table_disagreement_16_bits() {
    Fix f(16), g(16);
    // two keys under spec whose paths share a 16-bit hash at seed 0: each object is fine alone, the tables disagree
    auto leaf_hash = [&](const std::string& o) -> uint64_t {  // ~0: not valid alone (e.g. the leaf collides with "spec")
        CHECK(g.enc.flatten_json((const uint8_t*)o.data(), o.size(), g.an, g.fn));
        if (!g.enc.hash_single(g.fn, 0)) return ~0ull;
        CHECK(g.fn.spec.size() == 1);
        return g.fn.spec[0].h;
    };
    const std::string old_json = R"({"spec":{"a0":1}})";
    const uint64_t h = leaf_hash(old_json);
    CHECK(h != ~0ull);
    std::string new_json;
    for (int i = 0; i < (1 << 21) && new_json.empty(); i++) {
        const std::string o = "{\"spec\":{\"b" + std::to_string(i) + "\":1}}";
        if (leaf_hash(o) == h) new_json = o;
    }
    CHECK(!new_json.empty());
    PathTable told, tnew;
    CHECK(table_of(16, old_json, 0, &told) && table_of(16, new_json, 0, &tnew));
    CHECK(!tab_agree(tab_view(told), tab_view(tnew)));
    Tab tab;
    tab.t = &told;
    uint32_t want = 0;
    CHECK(g.enc.flatten_json((const uint8_t*)old_json.data(), old_json.size(), g.ao, g.fo) &&
          g.enc.flatten_json((const uint8_t*)new_json.data(), new_json.size(), g.an, g.fn) &&
          g.enc.pair_seed(g.fo, g.fn, &want));
    CHECK(want != 0);
    StoreDecision d = decide(f, true, 0, tab, &old_json, new_json);
    CHECK(d.rung == StoreRung::kReencodedOld && d.seed == want && d.store_ok && tab.calls == 1);
    counters(d, 1, 1, 0);
    // without old_json: conservative, and the new version is stored as it hashes alone
    d = decide(f, true, 0, tab, nullptr, new_json);
    CHECK(d.rung == StoreRung::kPairError && d.store_ok && d.seed == 0 && tab.calls == 1);
    counters(d, 0, 0, 1);
    CHECK(same_tab(f.fn.tab, tnew));
}

int main() {
    rungs_32_bits();
    forced_collisions_8_bits();
    table_disagreement_16_bits();
    std::printf("ok\n");
    return 0;
}
'''


def test_store_decide():
    csrc = os.path.join(ROOT, "kcp_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        exe = os.path.join(d, "t")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-I", csrc, src, os.path.join(csrc, "encoder.cpp"),
                        os.path.join(csrc, "json.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        assert r.stdout.strip() == "ok"
