// The Go-exact host marshaller of the write path (go_marshal.cpp): the request body of one decoded object, its
// descriptors, and the host-only entry points of include/gpudiff.h over them.  It is K10's oracle and completes the
// documents K10 defers (upsert.cpp).  Plain C++ over json.h and include/gpudiff.h, no HIP: this header and
// go_marshal.cpp include neither engine.h, tokenize.h, dstore.h, doc_batch.h nor a HIP header, directly or through
// another header -- the tests compile go_marshal.cpp and json.cpp into stand-alone programs under the sanitizers.
// Internal, not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/gpudiff.h"
#include "json.h"

namespace gd {

// a body's resourceVersion splice point (include/gpudiff.h GPUDIFF_RV_*)
struct RvSplice {
    uint32_t off = 0;
    uint32_t form = GPUDIFF_RV_NONE;
};
// a body's request target (include/gpudiff.h GPUDIFF_TGT_*): [0] metadata.name, [1] metadata.namespace
struct Targets {
    uint32_t off[2] = {0, 0};
    uint32_t len[2] = {0, 0};
    uint32_t flags = 0;
};
// the host path's descriptors of one body
struct HostDesc {
    RvSplice rv;
    Targets tgt;
};

// The body for one decoded object (root: a J_OBJ); *d (optional) = where its resourceVersion member would go, and
// where metadata.name's and metadata.namespace's values stand in it.
void upsert_body(const Node& root, uint32_t mode, std::string& o, HostDesc* d);
// The Update body for one decoded object: the transform of `mode`, then SetResourceVersion(rv), then the marshal --
// a direct marshal, not upsert_body and the splice: it is the independent answer the splice is compared against.
void update_body(const Node& root, uint32_t mode, const uint8_t* rv, size_t rv_len, std::string& o);
// Unstructured.GetName() / GetNamespace() of a decoded object: p / n [0] the name's bytes, [1] the namespace's
void target_strings(const Node& root, const char** p, size_t* n);
// host marshal of one document into o, its descriptors into *d; false = Go decode error
bool host_body(const uint8_t* doc, size_t len, uint32_t mode, std::string& o, HostDesc* d);
// Go's text of `f` (json's floatEncoder(64)) into out, its length returned: 32 bytes hold any float64 (24 digits and
// zeros, sign, "0.").  The value renderer's host formatter (valstr.h, devenc.cpp).
uint32_t go_float_text(double f, char* out);

}  // namespace gd
