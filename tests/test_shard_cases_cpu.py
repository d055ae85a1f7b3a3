"""CPU: the pieces tests/test_gpu_shard_step.py stands on (tests/shard_cases.py) -- the enumeration of contiguous splits, the
rank simulator over the float64 oracle against the oracle's unsharded loop for EVERY split of a 5-frame clip, and the two
references of the cross-rank sum: the float32 rank-ordered accumulator (the contract) stays within the standard bound of the
float64 sum, and on the cancellation rows its bits differ from the rounded float64 sum and from the reversed order -- so the
bit check on the device can tell a widened or reordered sum from the contract."""
import numpy as np
import pytest
import torch

from tests import shard_cases as sc


@pytest.mark.parametrize("N", [1, 2, 5, 6, 8])
def test_splits_are_all_the_contiguous_tilings(N):
    from smalify_amd import distributed
    got = sc.splits(N)
    assert len(got) == 2 ** (N - 1)
    assert len({tuple(s) for s in got}) == len(got)
    for s in got:
        assert s[0][0] == 0 and s[-1][1] == N
        assert all(lo < hi for lo, hi in s)
        assert all(s[i][1] == s[i + 1][0] for i in range(len(s) - 1))
    for world in range(1, N + 1):                      # shard_range's balanced split is one of them
        assert [distributed.shard_range(N, r, world) for r in range(world)] in got
    assert sc.split_of((1, 3, 1)) in sc.splits(5) and sc.split_name(sc.split_of((1, 3, 1))) == "1+3+1"


def test_variant_splits_are_splits():
    for n, sizes in sc.VARIANT_SPLITS.items():
        for s in sizes:
            assert sc.split_of(s) in sc.splits(n)


SIM_SCHEDULE = ((0, 2), (2, 2))


@pytest.fixture(scope="module")
def oracle_run():
    """the unsharded float64 oracle loop of the 5-frame, window-2 clip without silhouette (tests/test_distributed_cpu.py's
    problem and weights), once"""
    from oracle import smal_oracle as so
    from smalify_amd import config as cfg
    from tests import test_distributed_cpu as tdc
    torch.set_num_threads(2)
    prob, params = tdc._problem(5, 2)
    W = np.array(cfg.OPT_WEIGHTS).T
    weights = {s: W[s][:6].copy() for s, _ in SIM_SCHEDULE}
    weights[2][1] = 0.0                                # no silhouette
    ref = dict(params)
    for stage_id, its in SIM_SCHEDULE:
        opt = so.Adam(so.PARAM_ORDER, lr=float(W[stage_id][8]))
        for _ in range(its):
            _, _, grads = so.loss_and_grads(prob, ref, weights[stage_id], float(W[stage_id][6]), so.trainable_names(stage_id))
            opt.step(ref, grads)
    return prob, params, weights, W, {k: v.numpy() for k, v in ref.items()}


@pytest.mark.parametrize("split", sc.splits(5), ids=sc.split_name)
def test_rank_sim_over_the_oracle_reproduces_the_unsharded_loop(split, oracle_run):
    """every split of 5 frames with window 2: the simulator drives OracleLocalFitters through the generic protocol
    (evaluate / apply_adam / shared_grad / boundary_records) and must land on the unsharded float64 loop within the bound of
    test_distributed_cpu.py::test_sharded_fit_matches_single_process, shared parameters in the same bits on every rank"""
    prob, params, weights, W, ref = oracle_run
    sim = sc.RankSim([sc.OracleLocalFitter(prob, params, lo, hi, 2) for lo, hi in split])
    assert sim.generic
    for stage_id, its in SIM_SCHEDULE:
        sim.begin_stage(stage_id)
        for _ in range(its):
            sim.step(weights[stage_id], float(W[stage_id][6]), float(W[stage_id][8]), stage_id)
            assert len(sim.losses) == len(split) and tuple(sim.gather.shape) == (len(split), 26 + 216)
            for r, f in enumerate(sim.fitters):        # the halos are the neighbours' rows of the buffer, after the step
                rec = f.boundary_records()
                assert torch.equal(sim.gather[r, 26:].view(2, 108), rec)
                assert (f.halo_prev is None) == (r == 0) and (f.halo_next is None) == (r == len(split) - 1)
                if r > 0:
                    assert torch.equal(f.halo_prev, sim.fitters[r - 1].boundary_records()[1])
                if r + 1 < len(split):
                    assert torch.equal(f.halo_next, sim.fitters[r + 1].boundary_records()[0])
    got = sim.params()
    for k in ("betas", "log_beta_scales"):
        for r in range(len(split)):
            assert np.array_equal(got[r][k].numpy(), got[0][k].numpy()), (k, r)
            assert np.allclose(got[r][k].numpy(), ref[k], rtol=1e-9, atol=1e-12), (k, r)
    for k in ("global_rotation", "trans", "joint_rotations"):
        both = np.concatenate([g[k].numpy() for g in got], 0)
        assert np.allclose(both, ref[k], rtol=1e-9, atol=1e-12), k


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", sc.REDUCE_CASES, ids=lambda c: "w%d-ns%d-%s-%s-step%d" % c)
def test_the_contract_sum_is_within_the_standard_bound(case):
    c = sc.reduce_case(*case)
    rows = c["rows"]
    assert rows.dtype == np.float32 and rows.shape == (c["world"], c["ns"])
    got, ref = sc.rank_ordered_sum_f32(rows), sc.sum_f64(rows)
    assert got.dtype == np.float32
    assert (np.abs(got.astype(np.float64) - ref) <= sc.sum_bound(rows)).all()
    if c["world"] == 1:
        assert np.array_equal(_bits(got), _bits(rows[0]))
    # the case is what the GPU test needs: NaN in every float beyond ns, NaN moments at step 0 only, zero columns with zero moments
    g = c["gathered"]
    assert g.shape == (c["world"], c["stride"]) and np.isnan(g[:, c["ns"]:]).all() and np.isfinite(g[:, :c["ns"]]).all()
    assert np.isnan(c["exp_avg_in"][:c["ns"]]).all() == (c["step"] == 0) and np.isfinite(c["exp_avg"]).all()
    assert not got[c["zero"]].any() and not c["exp_avg"][:c["ns"]][c["zero"]].any() and not c["exp_avg_sq"][:c["ns"]][c["zero"]].any()
    assert 0 <= c["ntrain"] <= c["ns"] <= c["stride"]


def test_reduce_cases_cover_every_axis_and_the_corners():
    cases = sc.REDUCE_CASES
    for axis, values in enumerate((sc.REDUCE_WORLDS, sc.REDUCE_NUM_SHARED, sc.REDUCE_STRIDES, sc.REDUCE_TRAINED, sc.REDUCE_STEPS)):
        assert {c[axis] for c in cases} == set(values), axis
    assert (1, 26, "ns", "0", 0) in cases
    assert {sc.reduce_stride(26, k) for k in sc.REDUCE_STRIDES} == {26, 242, 279}
    assert set(sc.RECORD_NUM_SHARED) >= {40, 41} and (40 + 216) == 256


@pytest.mark.parametrize("world", [3, 8, 64])
def test_cancellation_rows_tell_the_contract_from_a_widened_or_reordered_sum(world):
    rows = sc.cancellation_rows(world)
    b = rows[2, 0]
    contract = sc.rank_ordered_sum_f32(rows)
    widened = sc.sum_f64(rows).astype(np.float32)
    reverse = sc.rank_ordered_sum_f32(rows[::-1])
    assert np.array_equal(_bits(widened), _bits([b, b]))
    assert np.array_equal(_bits(contract), _bits([b, 0.0]))
    assert _bits(contract)[1] != _bits(widened)[1]                 # float32 in rank order is not the rounded float64 sum
    assert _bits(contract)[0] != _bits(reverse)[0]                 # ... nor the same ranks added from the other end
    assert (np.abs(contract.astype(np.float64) - sc.sum_f64(rows)) <= sc.sum_bound(rows)).all()


def test_record_reference_layout():
    c = sc.record_case(26, 5)
    ref = sc.record_reference(26, **c)
    assert ref.dtype == np.float32 and ref.shape == (26 + 216,)
    assert np.array_equal(_bits(ref[:26]), _bits(c["shared_grad"][:26]))
    first, last = ref[26:134], ref[134:]
    assert np.array_equal(_bits(first[105:]), _bits(c["trans"][0])) and np.array_equal(_bits(last[105:]), _bits(c["trans"][4]))
    assert first[1] == 0.0 and last[1] == 0.0                       # the global mask's zero
    assert np.array_equal(_bits(last[3:105][c["rmask"] == 1]), _bits(c["jrot"][4][c["rmask"] == 1]))
    assert not last[3:105][c["rmask"] == 0].any()
    assert _bits(first[3])[()] == 0x80000000 and _bits(first[4])[()] == 0x80000000     # -0.0 under a one and under a zero
    assert first[5] == np.float32(1e-41) and first[5] != 0.0                            # a denormal stays one
    one = sc.record_reference(0, **sc.record_case(0, 1))
    assert one.shape == (216,) and np.array_equal(_bits(one[:108]), _bits(one[108:]))   # one frame: both blocks are that frame
