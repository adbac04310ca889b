"""Store what tests/test_robot_tables.py needs to regenerate the robot-table fixtures without the
reference tree: the two URDFs of make_robots.SOURCES, copied as they are, and the meshes of their
chains' links, thinned, under tests/golden/urdfs/ at the reference's relative paths.

The tables use a mesh only through the bounds of its raw points (robot_tables.mesh_box,
create_pz_bounding_boxes.m), so a thinned mesh keeps every triangle that carries one of the six
extreme coordinates and every KEEP-th other triangle: the same binary STL format, the same bounding
box to the bit, a few KB instead of up to 1.3 MB. Meshes of at most SMALL bytes are copied whole.

usage: python tests/golden/make_robot_meshes.py [reference root]"""
import os
import shutil
import struct
import sys
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_robots import SOURCES  # noqa: E402

KEEP = 64
SMALL = 16384
REC = np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])


def thin(src, dst):
    b = open(src, "rb").read()
    if len(b) <= SMALL:
        shutil.copyfile(src, dst)
        return
    n = struct.unpack("<I", b[80:84])[0]
    if len(b) != 84 + 50 * n:
        raise ValueError(f"{src}: not a binary STL")
    rec = np.frombuffer(b[84:], dtype=REC)
    v = rec["v"]                                     # [n][3 vertices][xyz]
    lo, hi = v.min(axis=(0, 1)), v.max(axis=(0, 1))
    keep = np.zeros(n, dtype=bool)
    keep[::KEEP] = True
    keep |= ((v == lo) | (v == hi)).any(axis=(1, 2))
    out = rec[keep]
    with open(dst, "wb") as f:
        f.write(b[:80] + struct.pack("<I", len(out)) + out.tobytes())
    w = out["v"]
    assert np.array_equal(w.min(axis=(0, 1)), lo) and np.array_equal(w.max(axis=(0, 1)), hi)


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    for urdf, _, _ in SOURCES.values():
        os.makedirs(os.path.dirname(os.path.join(HERE, urdf)), exist_ok=True)
        shutil.copyfile(os.path.join(ref, urdf), os.path.join(HERE, urdf))
        os.chmod(os.path.join(HERE, urdf), 0o644)
        meshes = {m.get("filename").replace("package://", "") for m in ET.parse(os.path.join(ref, urdf)).iter("mesh")}
        for m in sorted(meshes):
            src = os.path.join(ref, os.path.dirname(urdf), m)
            dst = os.path.join(HERE, os.path.dirname(urdf), m)
            if not os.path.exists(src):
                continue                             # robot_tables.mesh_box: the 10 cm default cube
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            thin(src, dst)
            os.chmod(dst, 0o644)
            print("wrote", os.path.relpath(dst, HERE), os.path.getsize(dst))
