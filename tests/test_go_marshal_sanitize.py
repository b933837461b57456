"""The Go-exact host marshaller (kcp_amd/csrc/go_marshal.cpp over json.cpp) as stand-alone programs under
AddressSanitizer / UndefinedBehaviorSanitizer -- no GPU needed: tools/update_body_sanitize.cpp and
tools/targets_sanitize.cpp, the second over the write path's test corpus.  That the two sources link with plain g++ is
the check that the marshaller needs no HIP header and nothing else of the library."""
import os
import struct
import subprocess

import pytest

from tests import upsert_cases as UC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kcp_amd", "csrc")
SAN = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _sanitizers_link(d):
    probe = os.path.join(d, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17"] + SAN + [probe, "-o", os.path.join(d, "probe")], capture_output=True)
    return r.returncode == 0


@pytest.fixture(scope="module")
def marshaller_objects(tmp_path_factory):
    """go_marshal.cpp and json.cpp compiled once, with the flags the programs get."""
    d = str(tmp_path_factory.mktemp("go_marshal"))
    if not _sanitizers_link(d):
        pytest.skip("g++ cannot link -fsanitize=address,undefined here: the marshaller's programs were not run")
    objs = []
    for name in ("go_marshal.cpp", "json.cpp"):
        objs.append(os.path.join(d, name + ".o"))
        subprocess.run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"), "-c",
                                                       os.path.join(CSRC, name), "-o", objs[-1]], check=True)
    return objs


def _run(tmp_path, objs, program, args=()):
    exe = os.path.join(str(tmp_path), "t")
    subprocess.run(["g++", "-std=c++17"] + SAN + ["-I" + os.path.join(ROOT, "include"),
                                                   os.path.join(ROOT, "tools", program)] + objs + ["-o", exe], check=True)
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
    print(r.stdout, end="")
    assert r.returncode == 0 and r.stdout.startswith("ok: "), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_update_body_program_under_sanitizers(tmp_path, marshaller_objects):
    out = _run(tmp_path, marshaller_objects, "update_body_sanitize.cpp")
    assert "known answers" in out and "refused descriptors" in out


def test_targets_program_under_sanitizers_over_the_corpus(tmp_path, marshaller_objects):
    docs = [k[1] for k in UC.KAT] + UC.fixture_docs() + UC.boundary_docs() + UC.synthetic_docs()
    corpus = os.path.join(str(tmp_path), "corpus.bin")
    with open(corpus, "wb") as f:
        f.write(b"".join(struct.pack("<I", len(x)) + x for x in docs))
    out = _run(tmp_path, marshaller_objects, "targets_sanitize.cpp", [corpus])
    assert "%d corpus documents" % len(docs) in out  # every document of the corpus was read and cross-checked
