#!/usr/bin/env python3
"""Generator of tests/golden/smal_template_mesh.npz: the geometry of the reference's SMAL template mesh
(smal_model/template_w_tex_uv.obj: 3889 vertices, 7774 faces), the one real SMAL-topology mesh the test-suite has -- every
other scene is the procedural stand-in (smalify_amd/data/synth_mesh.npz) or crafted triangles.

    python tests/golden/make_golden_template.py <reference tree>        (or SMALIFY_REFERENCE=<reference tree>)

What it stores (arrays only, none of the file's text):

  verts   float32 (3889, 3)   the `v` records, in file order
  faces   int16   (7774, 3)   the vertex index of each `f` record's three corners, zero-based, in file order
  source  a short tag naming the file the arrays were read from

No texture coordinates, normals, material names or comments.  It runs where the reference tree is; nothing else reads that
tree: tests/template_cases.py loads the npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "smal_template_mesh.npz")
OBJ = os.path.join("smal_model", "template_w_tex_uv.obj")
V, F = 3889, 7774


def read_obj(path):
    verts, faces = [], []
    with open(path) as fh:
        for line in fh:
            rec = line.split()
            if not rec:
                continue
            if rec[0] == "v":
                verts.append([float(x) for x in rec[1:4]])
            elif rec[0] == "f":
                assert len(rec) == 4, "a face that is no triangle: %r" % line
                faces.append([int(c.split("/")[0]) - 1 for c in rec[1:4]])
    return np.asarray(verts, np.float32), np.asarray(faces, np.int64)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SMALIFY_REFERENCE")
    if not ref or not os.path.isfile(os.path.join(ref, OBJ)):
        sys.exit("give the reference tree (the directory that holds %s) as the argument or in SMALIFY_REFERENCE: nothing written" % OBJ)
    verts, faces = read_obj(os.path.join(ref, OBJ))
    assert verts.shape == (V, 3) and faces.shape == (F, 3), (verts.shape, faces.shape)
    assert faces.min() == 0 and faces.max() == V - 1 and len(np.unique(faces)) == V
    np.savez_compressed(OUT, verts=verts, faces=faces.astype(np.int16), source=np.array("reference " + OBJ.replace(os.sep, "/") + ": v and f records"))
    kb = os.path.getsize(OUT) / 1024.0
    assert kb < 150.0, kb
    print("wrote %s (%.0f KB)" % (OUT, kb))


if __name__ == "__main__":
    main()
