"""kcp_amd/csrc/store_plan.h: the rules K17 / K19 (plan.hip) run, compiled into a stand-alone host program and run
over hand-made DocLink / flag tables -- no JSON, no GPU.  The chain fold's plan words are compared with the fold of
tests/store_plan_model.py; the body copy with memcpy, for every alignment of source and destination.  The program
is built with AddressSanitizer and UBSan (it has its own main): a walk or a copy that leaves its arrays fails."""
import os
import random
import subprocess

import pytest

from tests.store_plan_model import fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC_DIRTY, STATUS_DIRTY, DECODE_ERROR, SPEC_NOOP, STATUS_NOOP = 1, 2, 4, 8, 16
NO_ROW = 0xFFFFFFFF
W_SPEC, W_STATUS, W_SPEC_NOOP, W_STATUS_NOOP = 1, 2, 4, 8

SRC = r'''
#include "store_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace gd;

// stdin: "fold": nd nev kinds, then nd x (prev next row), then nev flags -> one plan word per document
static int run_fold() {
    unsigned nd, nev, kinds;
    if (std::scanf("%u %u %u", &nd, &nev, &kinds) != 3) return 2;
    std::vector<DocLink> links(nd);
    std::vector<uint8_t> flags(nev);
    for (unsigned i = 0; i < nd; i++) {
        long long prev, next, row;
        if (std::scanf("%lld %lld %lld", &prev, &next, &row) != 3) return 2;
        std::memset(&links[i], 0, sizeof(DocLink));
        links[i].prev = (int32_t)prev;
        links[i].next = (int32_t)next;
        links[i].row = (uint32_t)row;
    }
    for (unsigned i = 0; i < nev; i++) {
        unsigned f;
        if (std::scanf("%u", &f) != 1) return 2;
        flags[i] = (uint8_t)f;
    }
    for (unsigned i = 0; i < nd; i++) std::printf("%u\n", plan_word(links.data(), nd, flags.data(), nev, i, kinds));
    return 0;
}

// K19's copy: every (dst, src) offset 0..15 from an aligned block, lengths around every dword and wave boundary;
// 64 lanes one after the other; guard bytes around the destination must survive
static int run_copy() {
    const size_t lens[] = {0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 259, 260, 261, 1000, 1027};
    for (size_t n : lens)
        for (unsigned da = 0; da < 16; da++)
            for (unsigned sa = 0; sa < 16; sa++) {
                // exact-size heap blocks (the sanitizer sees any byte outside them); the source block is a
                // multiple of 4 B from an aligned start, as K10's arena slots are
                const size_t scap = (sa + n + 3) & ~(size_t)3;
                uint8_t* sbuf = (uint8_t*)std::malloc(scap ? scap : 4);
                uint8_t* dbuf = (uint8_t*)std::malloc(da + n + 16);
                if (((uintptr_t)sbuf | (uintptr_t)dbuf) & 7u) return 2;  // malloc: at least 8-B aligned
                for (size_t i = 0; i < scap; i++) sbuf[i] = (uint8_t)(i * 131 + 7 + n);
                std::memset(dbuf, 0xEE, da + n + 16);
                for (uint32_t lane = 0; lane < 64; lane++) plan_copy_body(dbuf + da, sbuf + sa, n, lane);
                bool ok = std::memcmp(dbuf + da, sbuf + sa, n) == 0;
                for (size_t i = 0; i < da; i++) ok = ok && dbuf[i] == 0xEE;
                for (size_t i = da + n; i < da + n + 16; i++) ok = ok && dbuf[i] == 0xEE;
                std::free(sbuf);
                std::free(dbuf);
                if (!ok) {
                    std::printf("copy failed: n=%zu dst%%16=%u src%%16=%u\n", n, da, sa);
                    return 1;
                }
            }
    std::printf("ok\n");
    return 0;
}

static int run_final_flags() {
    for (unsigned f = 0; f < 256; f++)
        for (unsigned nb = 0; nb < 4; nb++) std::printf("%u\n", plan_final_flags((uint8_t)f, (uint8_t)nb));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "fold")) return run_fold();
    if (!std::strcmp(argv[1], "copy")) return run_copy();
    if (!std::strcmp(argv[1], "flags")) return run_final_flags();
    return 2;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("store_plan_rule")
    src, out = str(d / "t.cpp"), str(d / "t")
    with open(src, "w") as f:
        f.write(SRC)
    # host only: store_plan.h's functions are __host__ __device__, and the sanitizers are for host code
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                    "-I", os.path.join(ROOT, "kcp_amd", "csrc"), "-I", os.path.join(ROOT, "include"), src, "-o", out],
                   check=True)
    return out


class Table:
    """A batch's document table, built the way dstore.cpp's add_doc chains documents."""

    def __init__(self):
        self.links, self.flags, self.last = [], [], {}

    def doc(self, slot, row):
        i = len(self.links)
        prev = self.last.get(slot, -1)
        if prev >= 0:
            self.links[prev][1] = i
        self.links.append([prev, -1, row])
        self.last[slot] = i
        return i

    def event(self, slot, flags, old_doc=False):
        if old_doc:  # a first sighting's old_json document: no row
            self.doc(slot, NO_ROW)
        row = len(self.flags)
        self.flags.append(flags)
        return self.doc(slot, row)


def _want(table, kinds):
    """Per document, the plan word by the model's fold over the chain's events."""
    out = [0] * len(table.links)
    for slot, tail in table.last.items():
        rows, d = [], tail
        while d >= 0:
            if table.links[d][2] != NO_ROW:
                rows.append(table.links[d][2])
            d = table.links[d][0]
        fl = [table.flags[r] for r in reversed(rows)]
        res = fold([dict(spec_dirty=bool(f & SPEC_DIRTY), spec_noop=bool(f & SPEC_NOOP),
                         status_dirty=bool(f & STATUS_DIRTY), status_noop=bool(f & STATUS_NOOP)) for f in fl])
        w = 0
        if kinds & 1 and res[0][0]:
            w |= W_SPEC | (W_SPEC_NOOP if res[0][1] else 0)
        if kinds & 2 and res[1][0]:
            w |= W_STATUS | (W_STATUS_NOOP if res[1][1] else 0)
        if table.links[tail][2] != NO_ROW:
            out[tail] = w
    return out


def _run_fold(exe, table, kinds):
    text = "%d %d %d\n" % (len(table.links), len(table.flags), kinds)
    text += "".join("%d %d %d\n" % tuple(l) for l in table.links) + " ".join(map(str, table.flags)) + "\n"
    r = subprocess.run([exe, "fold"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [int(x) for x in r.stdout.split()]


FLAG_CHOICES = [0, SPEC_DIRTY, STATUS_DIRTY, SPEC_DIRTY | STATUS_DIRTY, SPEC_DIRTY | SPEC_NOOP,
                STATUS_DIRTY | STATUS_NOOP, SPEC_DIRTY | STATUS_DIRTY | SPEC_NOOP,
                SPEC_DIRTY | STATUS_DIRTY | STATUS_NOOP, SPEC_DIRTY | STATUS_DIRTY | SPEC_NOOP | STATUS_NOOP,
                SPEC_DIRTY | STATUS_DIRTY | DECODE_ERROR]


def test_chain_fold_matches_model(exe):
    rnd = random.Random(17)
    t = Table()
    t.event(0, SPEC_DIRTY)                                    # length 1
    t.event(1, SPEC_DIRTY | SPEC_NOOP, old_doc=True)          # a head with row == kNoRow, then length 2
    t.event(1, 0)
    t.event(2, 0, old_doc=True)                               # all clean
    t.event(2, 0)
    t.event(3, STATUS_DIRTY | STATUS_NOOP)                    # no-op then real
    t.event(3, STATUS_DIRTY)
    for k in range(130):                                      # a chain of 130, interleaved with two others
        t.event(4, SPEC_DIRTY | SPEC_NOOP if k % 7 == 0 else 0, old_doc=k == 0)
        t.event(5, rnd.choice(FLAG_CHOICES))
        if k % 3 == 0:
            t.event(6, SPEC_DIRTY | SPEC_NOOP | (STATUS_DIRTY if k == 60 else 0))
    for _ in range(400):                                      # random interleaving over 25 slots
        s = 10 + rnd.randrange(25)
        t.event(s, rnd.choice(FLAG_CHOICES), old_doc=s not in t.last and rnd.random() < 0.5)
    assert len([1 for l in t.links if l[2] == NO_ROW]) >= 5
    for kinds in (3, 1, 2):
        got, want = _run_fold(exe, t, kinds), _want(t, kinds)
        assert got == want
        assert sum(1 for w in want if w) >= 20 and any(w & W_SPEC_NOOP for w in want) or kinds == 2
    # the 130-event chain: every dirty event a no-op, clean ones between -> one no-op spec write on its tail
    assert _want(t, 3)[t.last[4]] == W_SPEC | W_SPEC_NOOP
    assert _want(t, 3)[t.last[2]] == 0


def test_damaged_tables_stay_in_bounds(exe):
    """Links that point outside the table, rows past the flags and a prev cycle: the walk ends (the sanitizers
    see any read outside the arrays), it does not have to mean anything."""
    t = Table()
    t.event(0, SPEC_DIRTY)
    t.event(0, STATUS_DIRTY)
    t.event(1, SPEC_DIRTY)
    t.links[0][0] = 999          # prev outside the table
    t.links[2][0] = 2            # a cycle on itself
    t.links[2][2] = 77           # a row past the flags
    got = _run_fold(exe, t, 3)
    assert got[1] == W_SPEC | W_STATUS and got[2] == 0 and got[0] == 0


def test_final_flags_merge(exe):
    r = subprocess.run([exe, "flags"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in r.stdout.split()]
    k = 0
    for f in range(256):
        for nb in range(4):
            w = f & 7
            if not w & DECODE_ERROR:  # as api.cpp collect_results
                if nb & 1 and w & SPEC_DIRTY:
                    w |= SPEC_NOOP
                if nb & 2 and w & STATUS_DIRTY:
                    w |= STATUS_NOOP
            assert got[k] == w, (f, nb)
            k += 1


def test_body_copy_every_alignment(exe):
    r = subprocess.run([exe, "copy"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
