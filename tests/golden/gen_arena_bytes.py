#!/usr/bin/env python3
"""Generates tests/golden/arena_bytes.json: what the four arena sizing functions of the native executor
(imf_resunet_{int,float}_arena_bytes{,_cap}) return over a grid of descriptors and row counts.

    python tests/golden/gen_arena_bytes.py path/to/libimfnet_hip.so

The byte counts are part of the C ABI (callers allocate by them), so the record is taken from the library of the commit
BEFORE a change to the executor's layout code -- never from the code under test -- and
tests/test_cabi_and_host.py::test_arena_sizes_equal_the_recorded_ones holds every later build to it.  Host functions
only: runs without a GPU."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from imfnet_amd._lib import ResunetDesc  # noqa: E402

CHANNELS, TR_CHANNELS = [0, 32, 64, 128, 256], [0, 64, 64, 64, 128]       # ResUNetBN2C
DESCS = {"bn2c_k5": dict(in_channels=1, first_ksize=5, small_first=1),
         "bn2c_k3": dict(in_channels=1, first_ksize=3, small_first=1),
         "bn2c_k3_cin32": dict(in_channels=32, first_ksize=3, small_first=0)}
ROWS = [(1, 1, 1, 1), (63, 17, 5, 2), (64, 64, 64, 64), (65, 64, 1, 1), (4097, 1031, 263, 70),
        (103396, 27011, 7013, 1907)]
BBOX = (0, -40, -10, 3, 1, 120, 95, 60)                 # batch 0..1, x -40..120, y -10..95, z 3..60
GRID_WORDS = (4, 1 << 18)


def descriptor(in_channels, first_ksize, small_first):
    d = ResunetDesc()
    for i in range(5):
        d.channels[i], d.tr_channels[i] = CHANNELS[i], TR_CHANNELS[i]
    d.in_channels, d.out_channels, d.first_ksize, d.small_first = in_channels, 32, first_ksize, small_first
    return d


def sizes(handle):
    """[{desc, n, int_exact, int_exact_bbox, float_exact, int_cap: {words: bytes}, float_cap}] of the library `handle`."""
    P = C.c_void_p
    for name, args in (("imf_resunet_int_arena_bytes", [P, P, P]), ("imf_resunet_float_arena_bytes", [P, P]),
                       ("imf_resunet_int_arena_bytes_cap", [P, P, C.c_size_t]),
                       ("imf_resunet_float_arena_bytes_cap", [P, P])):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = C.c_size_t, args
    bbox = (C.c_int32 * 8)(*BBOX)
    out = []
    for name, kw in DESCS.items():
        d = C.byref(descriptor(**kw))
        for rows in ROWS:
            n = (C.c_int64 * 4)(*rows)
            out.append(dict(desc=name, n=list(rows),
                            int_exact=handle.imf_resunet_int_arena_bytes(d, n, None),
                            int_exact_bbox=handle.imf_resunet_int_arena_bytes(d, n, bbox),
                            float_exact=handle.imf_resunet_float_arena_bytes(d, n),
                            int_cap={str(w): handle.imf_resunet_int_arena_bytes_cap(d, n, w) for w in GRID_WORDS},
                            float_cap=handle.imf_resunet_float_arena_bytes_cap(d, n)))
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    record = dict(descs=DESCS, bbox=list(BBOX), entries=sizes(C.CDLL(os.path.abspath(sys.argv[1]))))
    path = os.path.join(HERE, "arena_bytes.json")
    with open(path, "w") as f:
        json.dump(record, f, indent=0)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(record["entries"]), "entries")


if __name__ == "__main__":
    main()
