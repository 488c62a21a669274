"""Record tests/golden/mesh_workspace.json: the byte counts the five workspace queries of the mesh export path return
over a grid of sizes (run BEFORE a change to a workspace layout, never after; needs the built library, no GPU):

    python tests/golden/make_golden_mesh_workspace.py

Calls only primx_mcubes_workspace, primx_texbake_components_workspace, primx_texbake_raster_workspace,
primx_meshclean_workspace and primx_meshdecim_workspace.  The grid holds, per size argument, the smallest accepted values,
one item less / exactly / one more than a block of 256 threads and than a block of PTS = 1024 items, 2^20 and 2^20 + 1 (the
one-workgroup scan then owns more than one block sum per thread) and the largest value the 2^31 guard still accepts.
tests/test_mesh_workspace_cpu.py holds the library to the file and REJECTED to its messages.  Data only.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "mesh_workspace.json")

EDGES = [1, 255, 256, 257, 1023, 1024, 1025, 1 << 20, (1 << 20) + 1]
I31 = 1 << 31
MC_MAX = (I31 - 1) // 12            # 3 * (n * 2 * 2) < 2^31
F3_MAX = (I31 - 1) // 3             # 3 * F < 2^31 (components), 3 * V < 2^31 (cleanup)
F9_MAX = (I31 - 1) // 9             # 9 * F < 2^31 (cleanup, decimation)
V10_MAX = (I31 - 1) // 10           # 10 * V < 2^31 (decimation)
ATLAS_MAX = 16384
NCELLS = 128 ** 3                   # cleanup: M = max(V, 3 F, GRID_CAP^3 + 1)


def _mesh_pairs(v_max):
    """(V, F) of cleanup and decimation: each argument over the grid against 0 and 1, V = F, F = 2 V, the guards."""
    sizes = [0] + EDGES
    out = [(v, f) for v in sizes for f in (0, 1)] + [(v, f) for f in sizes for v in (0, 1)]
    out += [(s, s) for s in EDGES] + [(s, 2 * s) for s in EDGES]
    out += [(100, 200), (1 << 22, 1 << 20), (1 << 22, 1 << 21), (v_max, 0), (0, F9_MAX), (v_max, F9_MAX)]
    return sorted(set(out))


def cases() -> dict:
    """{entry point: the argument tuples in front of the `bytes` pointer}."""
    mc = [(2, 2, 2), (16, 16, 16), (128, 128, 128), (256, 256, 256), (7, 9, 16), (8, 8, 16), (8, 8, 17), (9, 16, 15)]
    for s in EDGES[1:] + [MC_MAX]:      # 1 is refused: a lattice has two points per axis at least
        mc += [(s, 2, 2), (2, s, 2), (2, 2, s)]
    cc = [(f, 6) for f in [0] + EDGES] + [(100, u) for u in EDGES] + [(s, 3 * s) for s in EDGES]
    cc += [(100, 600), (F3_MAX, 1), (F3_MAX, I31 - 1), (0, I31 - 1)]
    at = [1, 255, 256, 257, 1023, 1024, 1025, ATLAS_MAX]   # 2^20 is past the atlas limit: (1024, 1024) has 2^20 texels
    rs = [(w, 1) for w in at] + [(1, h) for h in at] + [(s, s) for s in at]
    rs += [(31, 33), (32, 32), (25, 41), (1024, 1025), (1025, 1024), (ATLAS_MAX, 1023)]
    # cleanup: GRID_CAP^3 + 1 = 2097153 decides M for every pair with V <= 2^21 and 3 F <= 2^21 (all of the small ones)
    clean = _mesh_pairs(F3_MAX) + [(NCELLS, 0), (NCELLS + 1, 0), (NCELLS + 2, 0), (0, NCELLS // 3), (0, NCELLS // 3 + 1)]
    return {
        "primx_mcubes_workspace": sorted(set(mc)),
        "primx_texbake_components_workspace": sorted(set(cc)),
        "primx_texbake_raster_workspace": sorted(set(rs)),
        "primx_meshclean_workspace": sorted(set(clean)),
        "primx_meshdecim_workspace": _mesh_pairs(V10_MAX),
    }


# (entry point, arguments, substring of the message): the sizes the *_cpu.py tests of the mesh modules see refused, and the
# first value past every guard of the grid above
REJECTED = [
    ("primx_mcubes_workspace", (1, 16, 16), b">= 2"),
    ("primx_mcubes_workspace", (16, 1, 16), b">= 2"),
    ("primx_mcubes_workspace", (16, 16, 0), b">= 2"),
    ("primx_mcubes_workspace", (1024, 1024, 1024), b"2^31"),
    ("primx_mcubes_workspace", (MC_MAX + 1, 2, 2), b"2^31"),
    ("primx_texbake_components_workspace", (1 << 30, 6), b"2^31"),
    ("primx_texbake_components_workspace", (F3_MAX + 1, 6), b"2^31"),
    ("primx_texbake_components_workspace", (10, 0), b"U >= 1"),
    ("primx_texbake_components_workspace", (-1, 6), b">= 0"),
    ("primx_texbake_raster_workspace", (0, 16), b"[1, 16384]"),
    ("primx_texbake_raster_workspace", (16, 0), b"[1, 16384]"),
    ("primx_texbake_raster_workspace", (16385, 16), b"[1, 16384]"),
    ("primx_texbake_raster_workspace", (16, 1 << 20), b"[1, 16384]"),
    ("primx_meshclean_workspace", (-1, 200), b">= 0"),
    ("primx_meshclean_workspace", (100, -1), b">= 0"),
    ("primx_meshclean_workspace", (100, 1 << 29), b"2^31"),
    ("primx_meshclean_workspace", (F3_MAX + 1, 0), b"2^31"),
    ("primx_meshclean_workspace", (0, F9_MAX + 1), b"2^31"),
    ("primx_meshdecim_workspace", (-1, 200), b">= 0"),
    ("primx_meshdecim_workspace", (100, -1), b">= 0"),
    ("primx_meshdecim_workspace", (100, 1 << 29), b"2^31"),
    ("primx_meshdecim_workspace", (V10_MAX + 1, 0), b"2^31"),
    ("primx_meshdecim_workspace", (0, F9_MAX + 1), b"2^31"),
]


def measure(h) -> dict:
    """{entry point: [[*arguments, bytes], ...]} from the loaded library `h`."""
    out = {}
    for name, rows in cases().items():
        fn = getattr(h, name)
        got = []
        for args in rows:
            b = C.c_int64(-1)
            status = fn(*args, C.byref(b))
            assert status == 0, (name, args, h.primx_last_error())
            got.append([*args, b.value])
        out[name] = got
    return out


def main():
    sys.path.insert(0, ROOT)
    import topia_xl_amd._lib as L
    got = measure(L.load())
    with open(OUT, "w") as f:      # one row per line
        f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]"
                                   for k, rows in got.items()) + "\n}\n")
    print(OUT)


if __name__ == "__main__":
    main()
