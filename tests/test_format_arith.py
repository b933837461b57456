"""include/gpudiff_format.h is where the blob format's arithmetic is written down once: the host, the oracle and
the HIP kernels (dstore.hip, paths.hip) call the same functions.  A stand-alone host program (its own main, built
with AddressSanitizer and UBSan, nothing loaded into Python) includes the header once as C99 and once as C++17 and
checks gpudiff_seg_bytes / gpudiff_blob_body / gpudiff_meta_arena on edge values against literal numbers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the same table in both languages: X(expression, expected)
CASES = r'''
/* l = 0, arena = 0 */
X(gpudiff_seg_bytes(0u, 0u), 0ull)
X(gpudiff_blob_body(0u, 0u, 0u, 0u), 0ull)
/* no 32-bit wrap: (2^32 - 1) * 16 + (2^32 - 16) = 17 * 2^32 - 32 */
X(gpudiff_seg_bytes(4294967295u, 4294967280u), 73014444000ull)
X(gpudiff_seg_bytes(4294967295u, 0u), 68719476720ull)
X(gpudiff_seg_bytes(0u, 4294967280u), 4294967280ull)
/* twice that is 34 * 2^32 - 64, rounded up to the 128-B line: 34 * 2^32 */
X(gpudiff_blob_body(4294967295u, 4294967280u, 4294967295u, 4294967280u), 146028888064ull)
/* body sizes at 127 / 128 / 129: one segment's arena, leaves + arena, both segments */
X(gpudiff_blob_body(0u, 127u, 0u, 0u), 128ull)
X(gpudiff_blob_body(0u, 128u, 0u, 0u), 128ull)
X(gpudiff_blob_body(0u, 129u, 0u, 0u), 256ull)
X(gpudiff_blob_body(7u, 15u, 0u, 0u), 128ull)
X(gpudiff_blob_body(8u, 0u, 0u, 0u), 128ull)
X(gpudiff_blob_body(8u, 1u, 0u, 0u), 256ull)
X(gpudiff_blob_body(4u, 0u, 3u, 15u), 128ull)
X(gpudiff_blob_body(4u, 16u, 3u, 0u), 128ull)
X(gpudiff_blob_body(4u, 16u, 3u, 1u), 256ull)
X(gpudiff_blob_body(1u, 0u, 0u, 0u), 128ull)
/* string lengths 8 / 9 / 11 / 12 (and 13): the tail past the 8 inline bytes, rounded up to 4 */
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_STR, 0u)), 0ull)
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_STR, 8u)), 0ull)
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_STR, 9u)), 4ull)
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_STR, 11u)), 4ull)
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_STR, 12u)), 4ull)
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_STR, 13u)), 8ull)
X(gpudiff_meta_arena((9u << 3) | 5u), 4ull)
/* the longest length a meta word holds (29 bits), and a long value that is no string */
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_STR, 536870911u)), 536870904ull)
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_INT, 12u)), 0ull)
X(gpudiff_meta_arena(gpudiff_meta(GPUDIFF_TAG_FLOAT, 24u)), 0ull)
'''

C_PART = r'''
#include "gpudiff_format.h"
#include <stdio.h>
#ifdef __cplusplus
#error "this part is the header as C"
#endif
static int chk(const char* expr, unsigned long long got, unsigned long long want) {
    if (got != want) printf("C   %s = %llu, want %llu\n", expr, got, want);
    return got != want;
}
int check_as_c(void) {
    int bad = 0;
#define X(expr, want) bad += chk(#expr, (unsigned long long)(expr), (want));
#include "cases.inc"
#undef X
    return bad;
}
'''

CPP_PART = r'''
#include "gpudiff_format.h"
#include <cstdio>
extern "C" int check_as_c(void);
#ifndef GPUDIFF_HD
#error "gpudiff_format.h defines GPUDIFF_HD before its first function"
#endif
static int chk(const char* expr, unsigned long long got, unsigned long long want) {
    if (got != want) std::printf("C++ %s = %llu, want %llu\n", expr, got, want);
    return got != want;
}
int main() {
    int bad = check_as_c();
#define X(expr, want) bad += chk(#expr, (unsigned long long)(expr), (want));
#include "cases.inc"
#undef X
    if (!bad) std::printf("ok\n");
    return bad ? 1 : 0;
}
'''

SAN = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
       "-I", os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("format_arith")
    for name, text in (("cases.inc", CASES), ("as_c.c", C_PART), ("main.cpp", CPP_PART)):
        with open(str(d / name), "w") as f:
            f.write(text)
    subprocess.run(["gcc", "-std=c99"] + SAN + ["-I", str(d), "-c", str(d / "as_c.c"), "-o", str(d / "as_c.o")],
                   check=True)
    subprocess.run(["g++", "-std=c++17"] + SAN + ["-I", str(d), str(d / "main.cpp"), str(d / "as_c.o"), "-o",
                                                   str(d / "t")], check=True)
    return str(d / "t")


def test_format_arithmetic_edges_in_c_and_cpp(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert CASES.count("X(") >= 25


def test_device_code_calls_the_header():
    """dstore.hip and paths.hip hold no restatement of the header's functions (the kernels of kernels.hip /
    tokenize.hip keep theirs for now, each named beside the function it must equal)."""
    for name in ("dstore.hip", "paths.hip"):
        text = open(os.path.join(ROOT, "kcp_amd", "csrc", name), encoding="utf-8").read()
        assert "gpudiff_blob_body(" in text
        assert " seg_bytes(" not in text and " blob_body(" not in text
