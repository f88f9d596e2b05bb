"""The tuning surface of libkle (kle_set_tuning / kle_get_tuning) against
tests/golden/tuning_surface.json, recorded from the library as it was before
the keys moved into one table: every key's default, the return code of every
probe value, the refusal texts; and include/kle.h's key list against both.

The surface is read in a fresh process (this file run as a script), so the
defaults are the library's own and not what an earlier test left behind:

    python tests/test_tuning_surface.py pynama_amd/libkle.so > tests/golden/tuning_surface.json

records the fixture (the keys are the fields of struct Tuning)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tuning_surface.json")
PROBE = (list(range(-2, 131)) + [639, 640, 641, 4095, 4096, 4097, 65535, 65536, 65537, 131072, 2000000,
                                 2 ** 30, 2 ** 31 - 1])
UNKNOWN = "no_such_key"
SET_ONLY = "spmv_sym_probe_ts"  # probe build only, and never readable


def struct_keys():
    src = open(os.path.join(ROOT, "pynama_amd", "csrc", "kle_internal.hpp")).read()
    body = src[src.index("struct Tuning {"):]
    body = re.sub(r"#ifdef KLE_PROBE_BUILD.*?#endif", "", body[:body.index("\n};")], flags=re.S)
    return re.findall(r"^\s*int (\w+) = ", body, flags=re.M)


def surface(libpath, keys):
    lib = C.CDLL(libpath)
    lib.kle_last_error.restype = C.c_char_p
    lib.kle_set_tuning.argtypes = [C.c_char_p, C.c_int]
    lib.kle_get_tuning.argtypes = [C.c_char_p, C.POINTER(C.c_int)]

    def get(key):
        v = C.c_int(-12345)
        rc = lib.kle_get_tuning(key.encode(), C.byref(v))
        return rc, v.value

    out = {"probe": PROBE, "keys": {}}
    for key in keys:
        rc, default = get(key)
        assert rc == 0, (key, rc)
        rcs, texts, held = [], set(), default
        for v in PROBE:
            rc = lib.kle_set_tuning(key.encode(), v)
            rcs.append(rc)
            if rc:
                texts.add(lib.kle_last_error().decode())
            else:
                held = v
            assert get(key) == (0, held), f"{key}: set {v} returned {rc}, get gives {get(key)}, expected {held}"
        assert len(texts) <= 1, (key, texts)
        assert lib.kle_set_tuning(key.encode(), default) == 0 and get(key) == (0, default), key
        out["keys"][key] = {"default": default, "rc": rcs, "error": texts.pop() if texts else None}
    for key in keys:  # (no key's probes moved another key)
        assert get(key) == (0, out["keys"][key]["default"]), key
    out["unknown_set"] = [lib.kle_set_tuning(UNKNOWN.encode(), 0), lib.kle_last_error().decode()]
    out["unknown_get"] = [get(UNKNOWN)[0], lib.kle_last_error().decode()]
    out["get_set_only"] = [get(SET_ONLY)[0], lib.kle_last_error().decode()]
    out["null_key_set"] = [lib.kle_set_tuning(None, 0), lib.kle_last_error().decode()]
    out["null_key_get"] = [lib.kle_get_tuning(None, C.byref(C.c_int())), lib.kle_last_error().decode()]
    out["null_value_get"] = [lib.kle_get_tuning(keys[0].encode(), None), lib.kle_last_error().decode()]
    return out


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def pa():
    import pynama_amd
    pynama_amd.load()
    return pynama_amd


def header_keys():
    hdr = open(os.path.join(ROOT, "include", "kle.h")).read()
    doc = hdr[hdr.index("const char *kle_last_error(void);"):hdr.index("int kle_set_tuning(")]
    return re.findall(r'"([a-z0-9_]+)"', doc)


def test_surface_is_the_recorded_one(pa, golden):
    assert golden["probe"] == PROBE and len(golden["keys"]) == 45
    run = subprocess.run([sys.executable, os.path.abspath(__file__), pa._lib.LIBPATH] + list(golden["keys"]),
                         capture_output=True, text=True, timeout=120)
    # (the child asserts too: a refused set leaves the value, every key ends at its default)
    assert run.returncode == 0, run.stderr[-2000:]
    now = json.loads(run.stdout)
    assert sorted(now) == sorted(golden)
    for key, want in golden["keys"].items():
        got = now["keys"][key]
        assert got["default"] == want["default"], key
        assert got["error"] == want["error"], key
        differ = [(v, a, b) for v, a, b in zip(PROBE, got["rc"], want["rc"]) if a != b]
        assert not differ, f"{key}: (value, rc now, rc recorded) {differ[:8]}"
    for name in golden:
        assert now[name] == golden[name], name
    assert now["get_set_only"][0] != 0 and now["unknown_set"][0] != 0


def test_struct_keys_are_the_recorded_ones(golden):
    assert sorted(struct_keys()) == sorted(golden["keys"])


def test_header_lists_every_key(pa, golden):
    listed = header_keys()  # (a key may be quoted again inside another's entry)
    for key in golden["keys"]:
        assert key in listed, f'include/kle.h does not list "{key}"'
    for key in set(listed):
        pa.runtime.get_tuning(key)  # raises on a key the library does not know


if __name__ == "__main__":
    json.dump(surface(sys.argv[1], sys.argv[2:] or struct_keys()), sys.stdout, separators=(",", ":"))
    sys.stdout.write("\n")
