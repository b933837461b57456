"""What the document-batch tests of the K10, K11 and K13 families share (tests/test_gpu_upsert.py,
test_gpu_rollup.py, test_gpu_negotiate.py: test_doc_batch_every_branch)."""

TOK_MAX_LEN = (1 << 24) - 64  # tokenize.h kTokMaxLen


def oversize(doc: bytes) -> bytes:
    """`doc` (its first comma a top-level one) padded with spaces behind that comma to kTokMaxLen + 1 bytes, the
    smallest length a document batch leaves out of the staged JSON: the same object to Go's decoder."""
    i = doc.index(b",") + 1
    out = doc[:i] + b" " * (TOK_MAX_LEN + 1 - len(doc)) + doc[i:]
    assert len(out) == TOK_MAX_LEN + 1
    return out
