"""The host-side size / layout queries of the conv launchers over a fixed grid of shapes (ctypes only: no torch, no
device). Callers size workspaces with these and the launchers lay them out with the same planning functions, so their
values are pinned: tests/host_queries_expected.json was written by ``--write`` from the tree before the launch planning
was gathered into one geometry function per kernel family, and tests/test_host_queries.py compares the tree to it.
Usage: python tools/host_queries.py --write | --check   (U3D_LIB names another build of the library)"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("U3D_LIB") or os.path.join(REPO, "multimodal-pl_amd", "u3d", "libu3d.so")
EXPECTED = os.path.join(REPO, "tests", "host_queries_expected.json")

NS = (1, 2, 3, 8)
DHW = ((1, 1, 1), (4, 7, 31), (5, 9, 33), (9, 5, 70), (33, 16, 16), (14, 17, 24), (24, 24, 24), (96, 96, 96))
CHANNELS = ((24, 24), (40, 48), (64, 128), (256, 256), (288, 64))  # (cin, cout) of the brick / implicit-GEMM queries
KS = ((3, 1), (3, 2), (1, 1))  # (ksize, stride) of u3d_conv_wgrad_splits
# option sets: the defaults, then one option changed at a time (restored afterwards)
OPTION_SETS = {"default": None, "RING_WGS=7": ("RING_WGS", 7), "RING_SC=4": ("RING_SC", 4),
               "CONVG_BW8=0": ("CONVG_BW8", 0), "CONVG_BW8=1": ("CONVG_BW8", 1), "CONVG_PERSIST=0": ("CONVG_PERSIST", 0)}

SHAPES = [(n, *s) for n in NS for s in DHW]
SHAPES_C = [(n, *s, ci, co) for n in NS for s in DHW for ci, co in CHANNELS]
# entry point -> argument tuples, in the order the values are stored
QUERIES = {
    "u3d_conv32_ring_wps": SHAPES,
    "u3d_conv32_ring_stats_ws_floats": [(n,) for n in NS],
    "u3d_conv32_ring_q_stats_ws_floats": SHAPES,
    "u3d_conv32_ring_q_queue_bytes": SHAPES,
    "u3d_convg_brick_gn_nparts": [(n, ci, d, h, w, co) for n, d, h, w, ci, co in SHAPES_C],
    "u3d_convg_brick_stats_ws_floats": [(n, d, h, w, co) for n, d, h, w, _, co in SHAPES_C],
    "u3d_conv_wgrad_splits": [(n, ci, d, h, w, co, k, s) for n, d, h, w, ci, co in SHAPES_C for k, s in KS],
}


def load(path=LIB):
    h = ctypes.CDLL(path)
    for name, rows in QUERIES.items():
        f = getattr(h, name)
        f.argtypes = [ctypes.c_int] * len(rows[0])
        f.restype = ctypes.c_longlong if name == "u3d_convg_brick_stats_ws_floats" else ctypes.c_int
    h.u3d_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int]
    h.u3d_get_option.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    return h


def collect(h, option):
    """{entry point: [value per argument tuple]} with `option` = None or (name, value) set for the duration."""
    old = ctypes.c_int(0)
    if option:
        name = option[0].encode()
        if h.u3d_get_option(name, ctypes.byref(old)) != 0 or h.u3d_set_option(name, option[1]) != 0:
            raise RuntimeError(f"option {option[0]} unknown to this library")
    try:
        return {q: [getattr(h, q)(*a) for a in rows] for q, rows in QUERIES.items()}
    finally:
        if option:
            h.u3d_set_option(name, old.value)


def collect_all(h):
    return {key: collect(h, option) for key, option in OPTION_SETS.items()}


def mismatches(got, want):
    """[(entry point, argument tuple, got, want)] of one option set's values."""
    out = []
    for q, rows in QUERIES.items():
        g, w = got[q], want.get(q, [])
        if len(g) != len(w):
            out.append((q, None, len(g), len(w)))
            continue
        out += [(q, a, x, y) for a, x, y in zip(rows, g, w) if x != y]
    return out


def main(argv):
    got = collect_all(load())
    if "--write" in argv:
        with open(EXPECTED, "w") as f:
            f.write("{\n" + ",\n".join(
                f' "{key}": {{\n' + ",\n".join(f'  "{q}": {json.dumps(v, separators=(",", ":"))}' for q, v in qs.items())
                + "\n }" for key, qs in got.items()) + "\n}\n")
        print(f"wrote {EXPECTED}: {sum(len(v) for qs in got.values() for v in qs.values())} values")
        return 0
    if "--check" in argv:
        with open(EXPECTED) as f:
            want = json.load(f)
        bad = [(key, *m) for key in OPTION_SETS for m in mismatches(got[key], want.get(key, {}))]
        for key, q, a, x, y in bad[:40]:
            print(f"{key}: {q}{a} = {x}, expected {y}")
        print(f"{len(bad)} of {sum(len(v) for qs in got.values() for v in qs.values())} values differ")
        return 1 if bad else 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
