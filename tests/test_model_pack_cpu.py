"""CPU: the tables smalfit_model_create uploads (smalify_amd/csrc/smal_model_pack.h: pack_smal_model, model_tables), called
through tests/host_plan_shim.cpp on the stand-in and on the variants of tests/model_forms.py.

1. Byte identity: tests/golden/model_pack_digests.json holds a SHA-256 per table and one of the whole blob, taken from the
   packing code while it was still a part of smalfit_model_create (that code, lifted into a program of its own and compiled by g++
   -O2 without contraction or fast-math, fed the same models through numpy.save).  pack_smal_model reproduces every one.
2. Structure, against numpy and independent of the digests: the face order, the adjacency, both sparse forms, the rest joints,
   the limb-scale table.
3. The data refusals of smalfit_model_create, in their order."""
import dataclasses
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import smal_oracle as so
from tests import host_plan
from tests import model_forms as mf

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ("base", "valence", "weights8", "weights9", "regressor", "regressor_k1", "v3328", "v3056", "v4100", "nb48", "nb64")
DTYPES = {"vt": np.float32, "sd": np.float32, "pd": np.float32, "w_val": np.float32, "wc_val": np.float32, "jr_val": np.float32,
          "jrv_val": np.float32, "Jt": np.float32, "JS": np.float32}          # every other table: int32

PARENTS_TEXT = "parents must satisfy 0 <= parents[i] < i"
FACE_TEXT = "face index out of range"
LANDMARK_TEXT = "model has fewer vertices than the SMAL landmark ids"

_PACKS = {}


@pytest.fixture(scope="module")
def plan():
    return host_plan.load()


@pytest.fixture(scope="module")
def digests():
    with open(os.path.join(HERE, "golden", "model_pack_digests.json")) as f:
        return json.load(f)


def model(name):
    return mf.base() if name == "base" else mf.variant(name)


def packed(plan, name):
    """-> (dims, tables as typed arrays, offsets, blob, raw table bytes), packed once per model"""
    if name not in _PACKS:
        dims, raw, offsets, blob = plan.pack_model(model(name))
        tables = {k: np.frombuffer(v, DTYPES.get(k, np.int32)) for k, v in raw.items()}
        _PACKS[name] = (dims, tables, offsets, blob, raw)
    return _PACKS[name]


def test_the_digests_cover_these_models_and_tables(digests):
    assert sorted(digests) == sorted(MODELS)
    for name in MODELS:
        assert sorted(digests[name]["tables"]) == sorted(t for t in host_plan.MODEL_TABLES if t != "parents")


@pytest.mark.parametrize("name", MODELS)
def test_tables_and_blob_are_the_parents_byte_for_byte(plan, digests, name):
    dims, _, offsets, blob, raw = packed(plan, name)
    want = digests[name]
    assert dims == want["dims"]
    for t, sha in want["tables"].items():
        assert hashlib.sha256(raw[t]).hexdigest() == sha, t
    assert hashlib.sha256(blob).hexdigest() == want["blob"]
    # the blob is the tables in the order of model_tables, each at the next multiple of 256 bytes, zeros between
    end = 0
    for t in host_plan.MODEL_TABLES:
        assert offsets[t] == (end + 255) // 256 * 256
        assert not any(blob[end:offsets[t]])
        assert blob[offsets[t]:offsets[t] + len(raw[t])] == raw[t]
        end = offsets[t] + len(raw[t])
    assert end == len(blob)
    assert raw["parents"] == np.asarray(model(name).parents, np.int32).tobytes()


@pytest.mark.parametrize("name", MODELS)
def test_dims_and_planar_bases(plan, name):
    md = model(name)
    dims, t, _, _, _ = packed(plan, name)
    f = mf.facts(md)
    assert dims == dict(V=f["V"], Vp=f["Vp"], F=f["F"], NB=f["NB"], Kw=f["Kw"], Kj=f["Kj"])       # Kw, Kj: the largest row count
    V, Vp, NB = dims["V"], dims["Vp"], dims["NB"]
    for key, src, rows in (("vt", np.asarray(md.v_template, np.float32).reshape(1, V, 3), 1),
                           ("sd", np.asarray(md.shapedirs, np.float32).reshape(NB, V, 3), NB),
                           ("pd", np.asarray(md.posedirs, np.float32).reshape(306, V, 3), 306)):
        planar = t[key].reshape(rows, 3, Vp)
        assert np.array_equal(planar[:, :, :V], src.transpose(0, 2, 1)) and not planar[:, :, V:].any(), key


@pytest.mark.parametrize("name", MODELS)
def test_faces_follow_the_internal_order_and_every_corner_is_listed_once(plan, name):
    md = model(name)
    dims, t, _, _, _ = packed(plan, name)
    V, F = dims["V"], dims["F"]
    faces_int = t["faces_int"].reshape(F, 3)
    assert np.array_equal(faces_int, np.asarray(md.faces, np.int32)[mf.internal_face_order(md)])
    vf_off, vf_idx = t["vf_off"], t["vf_idx"]
    assert len(vf_off) == V + 1 and vf_off[0] == 0 and vf_off[V] == 3 * F and len(vf_idx) == 3 * F + 1
    assert vf_idx[3 * F] == 0                                                          # the padding entry
    assert np.array_equal(np.diff(vf_off), mf.corner_counts(md.faces, V))
    assert np.array_equal(np.sort(vf_idx[:3 * F]), np.arange(3 * F))                   # every corner exactly once
    owner = np.repeat(np.arange(V), np.diff(vf_off))
    assert np.array_equal(faces_int.reshape(-1)[vf_idx[:3 * F]], owner)                # ... under its own vertex
    rising = np.diff(vf_idx[:3 * F]) > 0
    seam = vf_off[1:V] - 1                                                             # (between two vertices' ranges: anything)
    rising[seam[(seam >= 0) & (seam < 3 * F - 1)]] = True
    assert rising.all()                                                                # ascending internal corner index


def test_vertices_without_a_face_have_empty_ranges(plan):
    _, t, _, _, _ = packed(plan, "valence")
    _, isolated = mf.valence_facts()
    assert len(isolated) == 4
    for v in isolated:
        assert t["vf_off"][v] == t["vf_off"][v + 1]
    assert t["vf_off"][-1] == t["vf_off"][-2]                                          # the last vertex: the padding entry is what is read


def _dense_from_ell(j, val, K, V, Vp):
    j, val = j.reshape(K, Vp), val.reshape(K, Vp)
    assert not j[:, V:].any() and not val[:, V:].any()
    dense = np.zeros((V, 35), np.float32)
    for c in range(K):
        live = val[c, :V] != 0
        assert not (dense[np.arange(V)[live], j[c, :V][live]] != 0).any()              # an entry is stored once
        dense[np.arange(V)[live], j[c, :V][live]] = val[c, :V][live]
        assert not j[c, :V][~live].any()
    return dense, j, val


def _dense_from_csc(off, v, val, V):
    assert len(off) == 36 and off[0] == 0
    dense = np.zeros((V, 35), np.float32)
    for jj in range(35):
        rows = v[off[jj]:off[jj + 1]]
        assert (np.diff(rows) > 0).all()                                               # ascending vertex order
        dense[rows, jj] = val[off[jj]:off[jj + 1]]
    return dense


@pytest.mark.parametrize("name", MODELS)
def test_both_sparse_forms_scatter_back_to_the_dense_matrices(plan, name):
    md = model(name)
    dims, t, _, _, _ = packed(plan, name)
    V, Vp = dims["V"], dims["Vp"]
    for dense, K, ell, csc in ((md.weights, dims["Kw"], ("w_j", "w_val"), ("wc_off", "wc_v", "wc_val")),
                               (md.J_regressor, dims["Kj"], ("jrv_j", "jrv_val"), ("jr_off", "jr_v", "jr_val"))):
        want = np.asarray(dense, np.float32)
        got, j, val = _dense_from_ell(t[ell[0]], t[ell[1]], K, V, Vp)
        assert np.array_equal(got, want), ell
        # a row's entries fill the first slots, in ascending joint order
        count = (want != 0).sum(1)
        assert np.array_equal((val[:, :V] != 0).sum(0), count)
        for c in range(1, K):
            both = count > c
            assert (j[c, :V][both] > j[c - 1, :V][both]).all()
        assert K == max(1, int(count.max()))
        off = t[csc[0]]
        assert off[35] == (want != 0).sum() == len(t[csc[1]]) == len(t[csc[2]])
        assert np.array_equal(_dense_from_csc(off, t[csc[1]], t[csc[2]], V), want), csc


def test_an_all_zero_matrix_gives_the_one_entry_csc(plan):
    md = mf.base()
    zero = dataclasses.replace(md, J_regressor=np.zeros_like(np.asarray(md.J_regressor, np.float32)))
    dims, raw, _, _ = plan.pack_model(zero)
    t = {k: np.frombuffer(v, DTYPES.get(k, np.int32)) for k, v in raw.items()}
    assert dims["Kj"] == 1
    assert not t["jr_off"].any() and len(t["jr_off"]) == 36
    assert t["jr_v"].tolist() == [0] and t["jr_val"].tolist() == [0.0]
    assert len(t["jrv_j"]) == len(t["jrv_val"]) == dims["Vp"] and not t["jrv_j"].any() and not t["jrv_val"].any()
    assert not t["Jt"].any() and not t["JS"].any()


@pytest.mark.parametrize("name", MODELS)
def test_rest_joints_are_the_float64_products_rounded_once(plan, name):
    """Jt = J_regressor^T v_template and JS = J_regressor^T shapedirs in float64, rounded to float32 once.  The factors are float32,
    so every product is exact in float64; the sum runs over a joint's vertices in ascending order, which the loop below repeats
    (numpy's own reductions sum pairwise), so the comparison is `==`"""
    md = model(name)
    dims, t, _, _, _ = packed(plan, name)
    V, NB = dims["V"], dims["NB"]
    jr = np.asarray(md.J_regressor, np.float32).astype(np.float64)                     # (V,35)
    x = np.concatenate([np.asarray(md.v_template, np.float32).astype(np.float64)[:, :, None],
                        np.asarray(md.shapedirs, np.float32).astype(np.float64).reshape(NB, V, 3).transpose(1, 2, 0)], 2)   # (V,3,1+NB)
    acc = np.zeros((35, 3, 1 + NB))
    for j in range(35):
        for v in np.nonzero(jr[:, j])[0]:
            acc[j] += jr[v, j] * x[v]
    assert np.array_equal(t["Jt"], acc[:, :, 0].reshape(105).astype(np.float32))
    assert np.array_equal(t["JS"].reshape(105, NB), acc[:, :, 1:].reshape(105, NB).astype(np.float32))
    # and the order aside: numpy's product agrees to the rounding of a float64 sum
    assert np.allclose(acc[:, :, 0], jr.T @ x[:, :, 0], rtol=0, atol=1e-12)


def test_limb_scale_table_is_the_oracles(plan):
    _, t, _, _, _ = packed(plan, "base")
    s = so.limb_scales(torch.arange(1.0, 7.0, dtype=torch.float64)[None])[0]           # exp(logscale[c]) where scale c applies, 1 elsewhere
    want = torch.log(s).round().to(torch.int32).numpy().reshape(105) - 1                # -> c, or -1
    assert sorted(set(want.tolist())) == [-1, 0, 1, 2, 3, 4, 5]
    assert np.array_equal(t["sidx"], want)


def test_default_landmarks_are_the_oracles(plan):
    assert plan.default_landmarks() == tuple(so.LANDMARKS)


def test_data_refusals_and_their_order(plan):
    md = mf.base()
    assert plan.model_desc_refusal(md) is None
    parents = np.asarray(md.parents, np.int32).copy()
    parents[5] = 5
    faces = np.asarray(md.faces, np.int32).copy()
    faces[7, 1] = md.v_template.shape[0]
    neg = np.asarray(md.faces, np.int32).copy()
    neg[0, 0] = -1
    small = mf.verts_model(mf.MIN_VERTS)
    V = mf.MIN_VERTS - 1
    col = np.arange(3 * V)
    short = dataclasses.replace(small, v_template=small.v_template[:V], shapedirs=small.shapedirs[:, col], posedirs=small.posedirs[:, col],
                                weights=small.weights[:V], J_regressor=small.J_regressor[:V],
                                faces=np.ascontiguousarray(small.faces[(np.asarray(small.faces) < V).all(1)]))
    assert plan.model_desc_refusal(dataclasses.replace(md, parents=parents)) == PARENTS_TEXT
    assert plan.model_desc_refusal(dataclasses.replace(md, faces=faces)) == FACE_TEXT
    assert plan.model_desc_refusal(dataclasses.replace(md, faces=neg)) == FACE_TEXT
    assert plan.model_desc_refusal(short) == LANDMARK_TEXT
    assert plan.model_desc_refusal(small) is None                                      # the smallest model accepted
    # two faults at once: parents before faces before landmarks
    assert plan.model_desc_refusal(dataclasses.replace(md, parents=parents, faces=faces)) == PARENTS_TEXT
    short_bad_face = np.asarray(short.faces, np.int32).copy()
    short_bad_face[3, 2] = V
    assert plan.model_desc_refusal(dataclasses.replace(short, faces=short_bad_face)) == FACE_TEXT
    assert plan.model_desc_refusal(dataclasses.replace(short, parents=parents)) == PARENTS_TEXT
