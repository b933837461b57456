"""Shared by tests/test_path_values.py and tests/test_gpu_path_values.py: the edge pairs of the value renderer
(kcp_amd/csrc/valstr.h, kernels K21 / K22) as raw JSON documents.  What they must render to is the model's answer
(tests/path_values_model.py); nothing here states a text."""
import json


def _J(o) -> bytes:
    return json.dumps(o, separators=(",", ":"), ensure_ascii=False).encode("utf-8")


def _obj(spec=None, status=None, **top):
    o = {"apiVersion": "v1", "kind": "Edge", "metadata": {"name": "e"}}
    if spec is not None:
        o["spec"] = spec
    if status is not None:
        o["status"] = status
    o.update(top)
    return o


def _pair(spec_a, spec_b, status_a=None, status_b=None):
    return _J(_obj(spec_a, status_a)), _J(_obj(spec_b, status_b))


STRING_LENGTHS = (0, 1, 7, 8, 9, 11, 12, 13, 63, 64, 65, 255, 70000)


def _fill(n, salt):
    """n ASCII bytes without escapes, different for every salt."""
    return "".join(chr(ord("a") + (i * 7 + salt) % 26) for i in range(n))


def _strings():
    a = {"len%d" % n: _fill(n, 0) for n in STRING_LENGTHS}
    b = {"len%d" % n: (_fill(n, 1) if n else "x") for n in STRING_LENGTHS}
    b["len0"], a["len0b"], b["len0b"] = "nonempty", "was", ""  # the empty string on either side
    return a, b


def _escapes():
    a, b = {}, {}
    for name, c in (("quote", '"'), ("newline", "\n"), ("lt", "<"), ("ctl", "\x01")):
        for at in (7, 8):
            a["%s-at%d" % (name, at)] = "a" * at + c + "zz"
            b["%s-at%d" % (name, at)] = "b" * at + c + c
    for name, c in (("ls", "\u2028"), ("ps", "\u2029")):
        for at in (5, 6, 7, 8):
            a["%s-at%d" % (name, at)] = "a" * at + c + "z"
            b["%s-at%d" % (name, at)] = "b" * at + c
    for at in (6, 7):  # a 3-byte character over byte 8
        a["cjk-at%d" % at] = "a" * at + "日" + "z"
        b["cjk-at%d" % at] = "a" * at + "本"
    for at in (5, 6, 7):  # a 4-byte character over byte 8
        a["emoji-at%d" % at] = "a" * at + "\U0001F600" + "z"
        b["emoji-at%d" % at] = "a" * at + "\U0001F601"
    for at in (5, 6, 7, 8):  # E2 80 / E2 81 sequences that are not U+2028 / U+2029
        a["near-at%d" % at] = "a" * at + "\u2027" + "\u2068"
        b["near-at%d" % at] = "a" * at + "\u202a" + "\u20a8"
    a["tail-ends-in-quote"], b["tail-ends-in-quote"] = "a" * 20 + '"', "b" * 21 + "\\"
    a["tail-ends-in-ls"], b["tail-ends-in-ls"] = "a" * 20 + "\u2028", "b" * 9 + "\u2029"
    a["tail-ends-in-amp"], b["tail-ends-in-amp"] = "a" * 63 + "&", "b" * 64 + ">"
    a["all-escapes"], b["all-escapes"] = '"\\\n\r\t<>&\x00\x1f\u2028\u2029' * 7, '\u2029\u2028&><\t\r\n\\"' * 9
    return a, b


INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

# raw number literals: (A, B) -- each an exact fast-path literal of K0 except where noted
_NUMBERS = [("zero", "0", "7"), ("minus-one", "-1", "1"), ("int-min", str(INT64_MIN), "0"),
            ("int-max", str(INT64_MAX), "0"), ("half", "0.5", "0.25"), ("e21", "1e21", "1e20"),
            ("big-f", "123456789012345680000.0", "12345678901234568000.0"), ("e-6", "1e-6", "1e-5"),
            ("e-7", "1e-7", "1e-8"), ("neg-zero", "-0.0", "1.5"), ("to-neg-zero", "2", "-0.0"),
            ("int-to-float", "3", "3.0"), ("float-to-int", "4.0", "4")]


def _numbers():
    a = "{" + ",".join('"%s":%s' % (n, x) for n, x, _y in _NUMBERS) + "}"
    b = "{" + ",".join('"%s":%s' % (n, y) for n, _x, y in _NUMBERS) + "}"
    head = '{"apiVersion":"v1","kind":"Edge","metadata":{"name":"e"},"spec":'
    return (head + a + "}").encode(), (head + b + "}").encode()


def _retypes():
    a = {"n": None, "f": False, "t": True, "o": {}, "l": [], "scalar": 1, "tree": {"y": [2, "deep"]},
         "gone": "removed", "gone-long": "r" * 30, "same": "unchanged-long-string"}
    b = {"n": False, "f": True, "t": None, "o": [], "l": {}, "scalar": {"y": [2, "deep"]}, "tree": "flat",
         "new": "added", "new-long": "n" * 31, "same": "unchanged-long-string"}
    return a, b


def _arena(n=200, extra=False):
    """n long-string members (9..40 bytes), every 7th changed; extra: B gains members, so the leaf indices differ."""
    a = {"m%03d" % i: _fill(9 + i % 32, i) for i in range(n)}
    b = dict(a)
    for i in range(0, n, 7):
        b["m%03d" % i] = _fill(9 + (i + 5) % 32, i + 1)
    if extra:
        for i in range(0, n, 3):
            b["m%03d-x" % i] = _fill(9 + i % 17, i + 2)
        for i in range(1, n, 11):
            del b["m%03d" % i]
    return a, b


def _many(n=150):
    a = {"k%03d" % i: (_fill(5 + i % 90, i) if i % 3 else i) for i in range(n)}
    b = {"k%03d" % i: (_fill(6 + i % 90, i + 3) if i % 3 else i + 1) for i in range(n)}
    return a, b


def _cases():
    out = []
    out.append(("strings",) + _pair(*_strings()))
    out.append(("escapes",) + _pair(*_escapes()))
    out.append(("numbers",) + _numbers())
    out.append(("retypes",) + _pair(*_retypes()))
    out.append(("added-all", _J(_obj({})), _J(_obj(_retypes()[1], {"s": "status-long-value", "n": 1}))))
    out.append(("removed-all", _J(_obj(_retypes()[0], {"s": "status-long-value", "n": 1})), _J(_obj({}, {}))))
    # B without status: the sentinel, and A's status leaves REMOVED with their old values
    out.append(("status-absent", _J(_obj({"r": 1}, {"phase": "Running", "message": "a long status message", "n": 3})),
                _J(_obj({"r": 1}))))
    out.append(("arena-200",) + _pair(*_arena()))
    out.append(("arena-200-shifted",) + _pair(*_arena(extra=True)))
    sa, sb = _arena(70)
    ta, tb = _arena(90, extra=True)
    out.append(("status-behind-spec-arena",) + _pair(sa, sb, ta, tb))
    out.append(("status-only-behind-spec-arena",) + _pair(sa, sa, ta, tb))
    out.append(("many-150",) + _pair(*_many(), {"ok": True}, {"ok": True}))  # status there and equal: no sentinel
    labels_a = {"metadata": {"name": "e", "labels": {"app": "x" * 20, "tier": "db"}, "annotations": {"note": "<b>"}}}
    labels_b = {"metadata": {"name": "e", "labels": {"app": "y" * 21, "tier": "web"}, "annotations": {"note": "&"}}}
    out.append(("labels", _J(_obj({"r": 1}, **labels_a)), _J(_obj({"r": 1}, **labels_b))))
    return out


# inside K0's exact subset: every value comes from K21 / K22 over K0-written blobs
DEVICE_CASES = _cases()

# K0 defers these (a float beyond its exact conversion, a key that needs decoding): the host-resolved path
HOST_CASES = [
    ("subnormal", b'{"apiVersion":"v1","kind":"Edge","spec":{"tiny":5e-324,"s":"long string next to it"}}',
     b'{"apiVersion":"v1","kind":"Edge","spec":{"tiny":2.2250738585072009e-308,"s":"long string next to it!"}}'),
    ("non-ascii-key",) + _pair({"é": "café \u2028 <long enough for the arena>", "日": 1},
                               {"é": "café \u2029 <long enough for the arena!>", "日": 1.0}),
    ("escaped-key", b'{"apiVersion":"v1","kind":"Edge","spec":{"a\\nb":"old value, a long one","k":[1]}}',
     b'{"apiVersion":"v1","kind":"Edge","spec":{"a\\nb":"new value, a long one","k":[]}}'),
]

ALL_CASES = DEVICE_CASES + HOST_CASES
