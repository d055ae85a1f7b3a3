"""GPU: smalfit_fit_eval_windows through Engine.fit_eval_windows -- one row of loss terms and one row of the shared parameters'
gradient per window of the sequence, from ONE evaluation -- against the float64 oracle's window_loss per group of
FitProblem.window_groups(), at S = 64 on the synthetic model.

Every configuration is evaluated once (module cache): smalfit_fit_eval, the new entry twice, smalfit_fit_eval again; the tests
below read that record.  Bars: those tests/test_gpu_parity.py::test_fitter_full holds for a whole evaluation -- a row's total
within 1e-4 relative, a gradient row within 2e-3 relative L2; a row that misses while the whole evaluation of the same state
passes is held to twice the deviation of the oracle run in float32 on that row instead (the table is printed)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import smal_oracle as so  # noqa: E402
from smalify_amd import _lib, config as cfg, engine as eng, model_io, synthetic  # noqa: E402
from tests import parity_cases as pc  # noqa: E402
from tests.parity_cases import dev, rel  # noqa: E402

S = 64
W_TABLE = np.array(cfg.OPT_WEIGHTS).T
PAD = 64                       # sentinel floats on either side of every row buffer
SENTINEL = -12345.5

# name: (M, window, frame_offset, total_frames, stage, w_sil = 0, logscale_mode, joint limits)
CONFIGS = {
    "ragged_last_window": (5, 2, 0, 0, 2, False, 1, False),
    "one_window_stage0": (4, 4, 0, 0, 0, False, 1, False),
    "window_larger_than_M": (3, 8, 0, 0, 2, True, 1, False),
    "single_frame": (1, 1, 0, 0, 2, False, 1, False),
    "shard_inside_unowned_window": (3, 3, 2, 8, 2, False, 1, False),
    "every_frame_a_window_17": (17, 1, 0, 0, 2, True, 1, False),
    "per_frame_scales_20dim_prior": (5, 2, 0, 0, 2, True, 2, False),
    "no_scales_stage0": (4, 4, 0, 0, 0, False, 0, False),
    "joint_limits": (3, 2, 0, 0, 1, True, 1, True),
}
_ENGINES = {}
_RUNS = {}


def _engine(kind):
    """engines of this module only (their priors and limit tables differ from the shared ones of tests/parity_cases.py)"""
    if kind not in _ENGINES:
        _, _, dm = pc.get_model()
        e = eng.Engine(dm, 17, S)
        e.set_pose_prior(*synthetic.synthetic_pose_prior())
        sp = synthetic.synthetic_shape_prior()
        if kind == "prior20":
            e.set_shape_prior(np.ascontiguousarray(sp[0][:20, :20]), np.ascontiguousarray(sp[1][:20]))
        else:
            e.set_shape_prior(*sp)
        if kind == "limits":
            e.set_joint_limits(*model_io.joint_limit_table())
        _ENGINES[kind] = e
    return _ENGINES[kind]


_SETUPS = {}


def _setup(name, dtype=torch.float64):
    if (name, dtype) not in _SETUPS:
        _SETUPS[(name, dtype)] = _build(name, dtype)
    return _SETUPS[(name, dtype)]


def _build(name, dtype):
    M, window, off, total, stage, no_sil, mode, limits = CONFIGS[name]
    weights = W_TABLE[stage][:6].copy()
    if no_sil:
        weights[1] = 0.0
    weights[4] = 40.0 if limits else 0.0                     # (as case_fit_limits)
    with_sil = weights[1] > 0
    base, cur, tg = pc.make_problem_cpu(M, S, window, seed=21 + M, with_sil=with_sil)
    cur = dict(cur)
    unity = mode == 1
    sp = synthetic.synthetic_shape_prior()
    prec, mean = (sp[0], sp[1]) if unity else (sp[0][:20, :20], sp[1][:20])
    pp = synthetic.synthetic_pose_prior()
    lim = model_io.joint_limit_table() if limits else None
    prob = so.FitProblem(base.m if dtype == torch.float64 else so.OracleModel(pc.get_oracle_model()[0], dtype=dtype), S, tg["tj"], tg["vis"],
                         tg["tsil"], pp[0], pp[1], pp[2], prec, mean, window, use_unity_prior=unity, dtype=dtype,
                         joint_limits=lim, frame_offset=off, total_frames=total or None)
    if mode == 2:
        cur["log_beta_scales"] = (0.15 * np.random.RandomState(5).randn(M, 6)).astype(np.float32)
    vis = tg["vis"]
    if stage == 0:
        vis = so.stage0_visibility(torch.from_numpy(vis).double()).numpy().astype(np.float32)
    return prob, cur, tg, vis, weights, mode


def _oracle_rows(name, dtype=torch.float64):
    """per group of window_groups(): the nine terms, and the gradient of their sum with respect to betas / log_beta_scales"""
    prob, cur, tg, vis, weights, mode = _setup(name, dtype)
    rows, gb, gls = [], [], []
    for br, full, owned in prob.window_groups():
        leaf = {k: torch.from_numpy(v).to(dtype) for k, v in cur.items()}
        if mode == 0:
            leaf["log_beta_scales"] = torch.zeros(6, dtype=dtype)
        leaf["betas"].requires_grad_(True)
        leaf["log_beta_scales"].requires_grad_(True)
        total, terms = so.window_loss(prob, leaf, br, weights, torch.from_numpy(vis).to(dtype), None, full, owned)
        total.backward()
        t = {k: float(v.detach()) for k, v in terms.items()}
        rows.append([t.get("joint", 0.0), t.get("pose", 0.0), t.get("splay", 0.0), t.get("betas", 0.0), t.get("sil_reproj", 0.0),
                     0.0, 0.0, 0.0, t.get("limit", 0.0)])
        gb.append(leaf["betas"].grad.double().numpy())
        g = leaf["log_beta_scales"].grad
        gls.append(None if g is None else g.double().numpy())
    return np.array(rows), np.array(gb), gls


def _padded(W, cols):
    buf = torch.full((2 * PAD + W * cols,), SENTINEL, device="cuda")
    return buf, buf[PAD:PAD + W * cols].view(W, cols)


def _run(name):
    if name in _RUNS:
        return _RUNS[name]
    M, window, off, total, stage, no_sil, mode, limits = CONFIGS[name]
    prob, cur, tg, vis, weights, mode = _setup(name)
    e = _engine("limits" if limits else ("prior26" if mode == 1 else "prior20"))
    d = {k: dev(v) for k, v in cur.items()}
    if mode == 0:
        d["log_beta_scales"] = None
    kw = dict(betas=d["betas"], log_beta_scales=d["log_beta_scales"], global_rotation=d["global_rotation"],
              joint_rotations=d["joint_rotations"], trans=d["trans"], target_joints=dev(tg["tj"]), target_visibility=dev(vis),
              target_sil=dev(tg["tsil"]) if weights[1] > 0 else None, weights=weights, w_temp=0.0, window=window, temporal=False,
              frame_offset=off, total_frames=total)
    cpu = lambda t: None if t is None else t.detach().cpu().numpy().copy()  # noqa: E731
    out = dict(mode=mode, W=len(prob.window_groups()))
    W = out["W"]

    def plain(tag):
        # every evaluation of the record starts from a forgotten raster cache: the cached depth bounds never change a result beyond
        # float32 summation noise (tests/test_gpu_parity.py::test_raster_cache_never_changes_results), but they do change bits
        e.reset_raster_cache()
        lpf = torch.full((M, 9), SENTINEL, device="cuda")
        losses, grads = e.fit_eval(losses_per_frame=lpf, **kw)
        out[tag] = dict(losses=cpu(losses), lpf=cpu(lpf), **{"g_" + k: cpu(v) for k, v in grads.items()})

    def windows(tag, with_lpf):
        e.reset_raster_cache()
        bufs = {"losses": _padded(W, 9), "betas": _padded(W, 20)}
        if mode == 1:
            bufs["log_beta_scales"] = _padded(W, 6)
        lpf = torch.full((M, 9), SENTINEL, device="cuda") if with_lpf else None
        losses, grads, rows, row_grads = e.fit_eval_windows(
            losses_per_frame=lpf, window_losses=bufs["losses"][1],
            window_grads={k: v[1] for k, v in bufs.items() if k != "losses"}, **kw)
        assert rows.data_ptr() == bufs["losses"][1].data_ptr()
        out[tag] = dict(losses=cpu(losses), lpf=cpu(lpf), rows=cpu(rows), row_grads={k: cpu(v) for k, v in row_grads.items()},
                        bufs={k: cpu(v[0]) for k, v in bufs.items()}, **{"g_" + k: cpu(v) for k, v in grads.items()})

    plain("plain0")
    windows("win1", True)
    windows("win2", False)
    plain("plain1")
    out["status"] = e.status()
    _RUNS[name] = out
    return out


_ORACLE = {}


def _oracle(name):
    if name not in _ORACLE:
        _ORACLE[name] = _oracle_rows(name)
    return _ORACLE[name]


def _held(name, what, got, bar, f32_dev):
    """`got` within `bar` of `want`, or within twice the float32 oracle's own deviation on that row (computed only then)"""
    print("%-32s %-22s deviation %.3e  bar %.1e" % (name, what, got, bar))
    if got < bar:
        return
    yard = 2.0 * f32_dev()
    print("%-32s %-22s float32 oracle yardstick (2 x its deviation) %.3e" % (name, what, yard))
    assert got < yard, (name, what, got, bar, yard)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_rows_match_the_oracles_window_groups(name):
    r = _run(name)
    rows_o, gb_o, gls_o = _oracle(name)
    assert r["status"] == 0
    win = r["win1"]
    assert win["rows"].shape == rows_o.shape == (r["W"], 9)
    f32 = {}

    def oracle32():
        if "v" not in f32:
            f32["v"] = _oracle_rows(name, torch.float32)
        return f32["v"]

    for w in range(r["W"]):
        tot_o = rows_o[w].sum()
        _held(name, "row %d total" % w, abs(win["rows"][w].astype(np.float64).sum() - tot_o) / abs(tot_o), 1e-4,
              lambda w=w: abs(oracle32()[0][w].sum() - tot_o) / abs(tot_o))
        # every term sits in its own column (a check of places, not of precision: the bar above holds the total)
        assert np.abs(win["rows"][w] - rows_o[w]).max() < 1e-3 * abs(tot_o), (w, win["rows"][w], rows_o[w])
        _held(name, "row %d d/d betas" % w, rel(win["row_grads"]["betas"][w], gb_o[w]), 2e-3,
              lambda w=w: rel(oracle32()[1][w], gb_o[w]))
        if r["mode"] == 1:
            _held(name, "row %d d/d log scales" % w, rel(win["row_grads"]["log_beta_scales"][w], gls_o[w]), 2e-3,
                  lambda w=w: rel(oracle32()[2][w], gls_o[w]))
    if r["mode"] != 1:
        assert "log_beta_scales" not in win["row_grads"]
    # a row this evaluation does not own has neither the prior's term nor (through the sum above) its gradient
    M, window, off = CONFIGS[name][:3]
    if off % window:
        assert win["rows"][0][3] == 0.0 and rows_o[0][3] == 0.0
        assert (win["rows"][1:, 3] > 0).all()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_rows_add_up_to_the_calls_own_totals(name):
    """columns of the loss rows and rows of each gradient, added in float64, against the call's own losses / g_betas /
    g_log_beta_scales: float32 rounding of at most W + 1 additions plus one final rounding"""
    r = _run(name)
    win, W = r["win1"], r["W"]
    eps = (W + 2) * 2.0 ** -24

    def check(rows, total, what):
        rows = rows.astype(np.float64)
        bound = eps * np.abs(rows).sum(axis=0)
        diff = np.abs(rows.sum(axis=0) - total.astype(np.float64))
        print(name, what, "max diff / bound", float((diff / np.maximum(bound, 1e-300)).max()))
        assert (diff <= bound).all(), (what, diff, bound)

    check(win["rows"], win["losses"], "losses")
    check(win["row_grads"]["betas"], win["g_betas"], "g_betas")
    if r["mode"] == 1:
        check(win["row_grads"]["log_beta_scales"], win["g_log_beta_scales"], "g_log_beta_scales")


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_same_bits_as_the_plain_call_and_no_state_left_behind(name):
    r = _run(name)
    p0, p1, w1, w2 = r["plain0"], r["plain1"], r["win1"], r["win2"]
    same = ["losses", "g_global_rotation", "g_joint_rotations", "g_trans", "lpf"]
    if r["mode"] == 2:
        same.append("g_log_beta_scales")                    # per frame by nature: the assembly's, as ever
    for k in same:
        assert np.array_equal(p0[k], w1[k]), k
    assert not (p0["lpf"] == SENTINEL).any()
    # two calls of the new entry: the same bits (the second without losses_per_frame: the new kernel cleared the counters itself)
    for k in ("losses", "rows", "g_betas", "g_global_rotation", "g_joint_rotations", "g_trans") + (("g_log_beta_scales",) if r["mode"] else ()):
        assert np.array_equal(w1[k], w2[k]), k
    for k in w1["row_grads"]:
        assert np.array_equal(w1["row_grads"][k], w2["row_grads"][k]), k
    # smalfit_fit_eval after it: the bits it gave before it, and its per-frame rows saw cleared counters
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k
    # the shared gradients of the two entry points are two orders of one sum
    assert rel(w1["g_betas"], p0["g_betas"]) < 1e-4
    if r["mode"] == 1:
        assert rel(w1["g_log_beta_scales"], p0["g_log_beta_scales"]) < 1e-4


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_writes_stay_inside_the_rows(name):
    r = _run(name)
    for tag in ("win1", "win2"):
        for k, cols in (("losses", 9), ("betas", 20), ("log_beta_scales", 6)):
            if k not in r[tag]["bufs"]:
                continue
            buf = r[tag]["bufs"][k]
            assert buf.shape == (2 * PAD + r["W"] * cols,)
            assert (buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all(), (tag, k)
            assert not (buf[PAD:-PAD] == SENTINEL).any(), (tag, k)


def test_temporal_columns_go_to_the_window_of_the_pairs_first_frame():
    M, window = 5, 2
    prob, cur, tg, vis, weights, mode = _setup("ragged_last_window")
    weights = weights.copy()
    weights[1] = 0.0
    w_temp = float(W_TABLE[2][6])
    e = _engine("prior26")
    d = {k: dev(v) for k, v in cur.items()}
    lpf = torch.zeros(M, 9, device="cuda")
    losses, grads, rows, _ = e.fit_eval_windows(
        betas=d["betas"], log_beta_scales=d["log_beta_scales"], global_rotation=d["global_rotation"],
        joint_rotations=d["joint_rotations"], trans=d["trans"], target_joints=dev(tg["tj"]), target_visibility=dev(vis), target_sil=None,
        weights=weights, w_temp=w_temp, window=window, temporal=True, losses_per_frame=lpf)
    assert e.status() == 0
    rows, lpf, losses = rows.cpu().numpy().astype(np.float64), lpf.cpu().numpy().astype(np.float64), losses.cpu().numpy().astype(np.float64)
    want = np.zeros((3, 3))
    for n in range(M - 1):
        pair = {k: torch.from_numpy(cur[k][n:n + 2]).double() for k in ("global_rotation", "joint_rotations", "trans")}
        want[n // window] += [float(v) for v in so.temporal_terms(pair, w_temp)]
    assert np.abs(rows[:, 5:8] - want).max() < 1e-4 * np.abs(want).max(), (rows[:, 5:8], want)
    assert want[2].sum() == 0.0 and (rows[2, 5:8] == 0.0).all()          # the last frame has no successor
    for w in range(3):
        assert np.allclose(rows[w], lpf[w * window:(w + 1) * window].sum(axis=0), rtol=1e-6, atol=1e-7)
    assert np.allclose(rows.sum(axis=0), losses, rtol=1e-6, atol=1e-7)


def test_refused_blocks_launch_nothing():
    """one refused block per refusal text: non-zero, the text in smalfit_last_error(), no output written, no status bit set"""
    from tests.test_window_rows_cpu import COUNT_TEXT, LOSSES_TEXT, SCALES_TEXT, SIZE_TEXT, SUBJECT_TEXT
    M, window = 4, 2
    e = _engine("prior20")
    fn = _lib.resolve(e.lib, "smalfit_fit_eval_windows")
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    assert e.status() == 0

    def attempt(text, edit_rows=None, **fit):
        base = dict(betas=z(20), log_beta_scales=z(M, 6), global_rotation=z(M, 3), joint_rotations=z(M, 34, 3), trans=z(M, 3),
                    target_joints=z(M, 25, 2), target_visibility=z(M, 25), target_sil=None, weights=(1, 0, 0, 0, 0, 0), w_temp=0.0,
                    window=window, temporal=False)
        base.update(fit)
        a, losses, grads, keep = e.build_fit_args(**base)
        out = [losses] + list(grads.values())
        rows, gb, gls = torch.empty(M, 9, device="cuda"), torch.empty(M, 20, device="cuda"), torch.empty(M, 6, device="cuda")
        for t in out + [rows, gb, gls]:
            t.fill_(SENTINEL)
        r = _lib.WindowRows()
        r.num_windows, r.losses, r.g_betas = eng.Engine.num_windows(a.num_frames, max(a.window, 1)), rows.data_ptr(), gb.data_ptr()
        if edit_rows:
            edit_rows(r, gls)
        rc = fn(e.handle, eng._stream(), C.byref(a), C.byref(r))
        torch.cuda.synchronize()
        if text is None:
            assert rc == 0, e.lib.smalfit_last_error()
            return
        assert rc != 0
        assert e.lib.smalfit_last_error().decode() == "smalfit_fit_eval_windows: " + text
        for t in out + [rows, gb, gls]:
            assert (t == SENTINEL).all()
        assert e.status() == 0

    attempt(None)

    def shrink(r, gls):
        r.struct_size -= 8
    attempt(SIZE_TEXT, shrink)
    attempt(LOSSES_TEXT, lambda r, gls: setattr(r, "losses", None))
    attempt(COUNT_TEXT, lambda r, gls: setattr(r, "num_windows", 3))
    attempt(SUBJECT_TEXT, lambda r, gls: setattr(r, "num_windows", M), betas=z(M, 20), subject_frames=1, window=1)
    attempt(SCALES_TEXT, lambda r, gls: setattr(r, "g_log_beta_scales", gls.data_ptr()))                       # logscale_mode 2
    attempt(SCALES_TEXT, lambda r, gls: setattr(r, "g_log_beta_scales", gls.data_ptr()), log_beta_scales=None)  # logscale_mode 0
    # ... and the binding checks what the library cannot: the extent of the row buffers
    kw = dict(betas=z(20), log_beta_scales=z(6), global_rotation=z(M, 3), joint_rotations=z(M, 34, 3), trans=z(M, 3),
              target_joints=z(M, 25, 2), target_visibility=z(M, 25), target_sil=None, weights=(1, 0, 0, 0, 0, 0), w_temp=0.0, window=window)
    with pytest.raises(eng.SmalfitError, match="one row per window"):
        e.fit_eval_windows(window_losses=z(3, 9), **kw)
    with pytest.raises(eng.SmalfitError, match="one row per window"):
        e.fit_eval_windows(window_grads={"betas": z(2, 21)}, **kw)
    with pytest.raises(eng.SmalfitError, match="shared log_beta_scales"):
        e.fit_eval_windows(window_grads={"log_beta_scales": z(2, 6)}, **dict(kw, log_beta_scales=z(M, 6)))
