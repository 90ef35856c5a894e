"""The dense kriging family on the GPU where a call has more than one chunk of systems, where a factorisation fails, and where a shared
gauge set is wider than 8 frames (cases: tests/krig_sys_cases.py, their CPU companion: tests/test_krig_sys_cases_cpu.py, DESIGN.md
section 24b).

  A  the models' outputs are bit for bit the same however models/classical.py _Systems chunks the call's systems
  B  the stages called for an interior sub-range of systems (f0 > 0) write those frames' rows only, and what they write agrees with
     the fp64 restatement
  C  a system whose factorisation meets a non-positive pivot falls back (gauge mean, alpha = 0, NaN variance / LOO / members / LOSO)
     without leaking anything non-finite into its neighbours
  D  krig_predict_kernel's second and third group of 8 frames of a shared set
  E  the fields of the systems descriptor that a stage does not read may be NULL: the same bits

Error bound of every comparison with a restatement, the rule of the classical baselines: device error <= max(32 e32, 1e-6) max|ref|,
with e32 the fp32 restatement's own error against fp64 relative to max|ref|, computed in the same test."""
import logging

import numpy as np
import pytest
import torch

import classical_ref as cr
import krig_sys_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _model(dev, **model):
    from p2igan_bench.models import build_generator
    return build_generator({"model": model}).to(dev)


def _tensors(name, dev):
    masked, masks = kc.inputs(name)
    return torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)


def _same(a, b):
    """Bit-for-bit equality with NaN positions compared as equal."""
    if a is None or b is None:
        return a is b
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _within(what, got, r64, r32):
    """NaN positions agree with the restatement's; the rest is within max(32 e32, 1e-6) max|ref|."""
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(r64)), (what, "NaN positions differ")
    top = float(np.nanmax(np.abs(r64)))
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(got - r64), initial=0.0))
        e32 = float(np.nanmax(np.abs(r32.astype(np.float64) - r64), initial=0.0)) / max(top, 1e-30)
    bound = max(32.0 * e32, 1e-6) * top
    print(f"{what}: device err {err:.3e}  e32 {e32:.3e}  bound {bound:.3e}  (max|ref| {top:.3e})")
    assert err <= bound, (what, err, bound)


def _run_entry(G, entry, x, m):
    """The tensors an entry point leaves behind, last_status last."""
    if entry == "forward":
        out = [G(x, m)]
    elif entry == "forward_uq":
        out = list(G.forward_uq(x, m))
    elif entry.startswith("ensemble"):
        b, t = x.shape[:2]
        out = list(G.forward_ensemble(x, m, int(entry[8:]), seed=kc.SEED, streams=torch.from_numpy(kc.streams_of(b, t))))
    else:
        res = getattr(G, entry)(x, m)
        out = [res.pred, res.var, res.status, res.z, res.pix, res.counts] + ([] if res.site is None else [res.site])
    return [o.clone() for o in out] + [G.last_status.clone()]


# ---- A: chunk invariance
@pytest.mark.parametrize("cid,entry", [(c, e) for c, (_, _, entries) in kc.CHUNK_CASES.items() for e in entries], ids=kc.chunk_case_ids())
def test_chunks_do_not_change_a_bit(dev, monkeypatch, cid, entry):
    from p2igan_bench.models import classical
    model, name, _ = kc.CHUNK_CASES[cid]
    nsys, r, np_, T = kc.systems_of(cid)
    x, m = _tensors(name, dev)
    G = _model(dev, **model)
    whole = _run_entry(G, entry, x, m)
    assert G.last_status.numel() == nsys and int(G.last_status.sum()) == 0
    cand = G.last_fit["cand"].cpu().tolist()
    flat = {kc.FLAT[name]} | ({2} if name == "shared" else set())
    assert [c < 0 for c in cand] == [b in flat for b in range(len(cand))]            # the degenerate sample is there, and is not sample 0
    if not entry.startswith("cross_validate"):
        assert bool(torch.isfinite(whole[0]).all())                                    # the prediction is finite everywhere
    if entry != "forward":
        assert bool(torch.isnan(whole[1]).any()) and not bool(torch.isnan(whole[1]).all())      # NaN rows sit next to finite ones
    for per, fb, by in kc.chunk_plan(cid, entry):
        monkeypatch.setattr(classical, "_FACTOR_BYTES", fb)
        got = _run_entry(G, entry, x, m)
        for k, (a, b) in enumerate(zip(whole, got)):
            assert _same(a, b), (cid, entry, f"per {per} (by the {by} bound)", f"output {k}")
        monkeypatch.undo()


# ---- the stages of one sub-range of systems, as models/classical.py KrigingGenerator._krige chains them
def _sentinel(shape, dev):
    return torch.full(shape, kc.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == kc.SENTINEL).all())


def _krig_stages(dev, x, m, model, params, shared, s0, ns, np_, cap, members, streams, cand=None):
    """Factor, solve, invert, variance, LOO, conditioning weights and members of systems s0 .. s0 + ns - 1 only; every call-wide
    output holds the sentinel (ens: the unconditional field inside the sub-range, the sentinel outside it) before."""
    from p2igan_bench import ops
    B, T, _, H, W = x.shape
    F, HW, R = B * T, H * W, (T if shared else 1)
    code = ops.KRIG_MODELS[model]
    pix, z, info = ops.krig_compact(x.reshape(B, T, H, W).contiguous(), m.reshape(B, T, H, W).contiguous(), cap)
    f0, nf = s0 * R, ns * R
    o = {"alpha": _sentinel((F, cap), dev), "mean": _sentinel((F,), dev), "var": _sentinel((F, HW), dev),
         "loo_pred": _sentinel((F, cap), dev), "loo_var": _sentinel((F, cap), dev), "ens": _sentinel((F, members, HW), dev)}
    amp, _ = ops.krig_cs_spectrum(params, cand, code, H, W, kc.EMBED)
    fields = torch.empty(F, members, HW, device=dev, dtype=torch.float32)
    ops.krig_cs_fields(amp, torch.from_numpy(streams).reshape(F).to(dev), kc.SEED, T, members, H, W, kc.EMBED, fields)
    o["ens"][f0:f0 + nf] = fields[f0:f0 + nf]
    work = torch.empty(ns * np_ * np_, device=dev, dtype=torch.float32)
    winv = torch.empty_like(work)
    call = ops.KrigSystems(pix, z, info, params, cand, code, R, T, np_, torch.zeros(F // R, device=dev, dtype=torch.int32))
    sys = call.chunk(s0, ns)
    ops.krig_factor(sys, work)
    sol = ops.krig_solve(sys, work, o["alpha"], o["mean"])
    ops.krig_invert(work, ns, np_, winv)
    ops.krig_variance(sys, winv, sol, H, W, o["var"])
    ops.krig_loo(sys, winv, sol, o["alpha"], o["loo_pred"], o["loo_var"])
    ca, cm = ops.krig_cs_weights(sys, winv, sol, o["ens"], members, H, W)
    ops.krig_cs_predict(sys, ca, cm, members, H, W, o["ens"])
    o["pred"] = ops.krig_predict(call.chunk(0, F // R), o["alpha"], o["mean"], H, W)       # every frame; outside: of the sentinel
    assert not call.status[:s0].any() and not call.status[s0 + ns:].any()
    o.update(status=sys.status, sol=sol, counts=info[:F].cpu().numpy(), f0=f0, nf=nf, R=R)
    return o


CALL_WIDE = ("alpha", "mean", "var", "loo_pred", "loo_var", "ens")


def _outside_is_untouched(o):
    f0, nf = o["f0"], o["nf"]
    for k in CALL_WIDE:
        assert _is_sentinel(o[k][:f0]) and _is_sentinel(o[k][f0 + nf:]), (k, "a row outside the sub-range was written")


# ---- B: a sub-range with f0 > 0 against the restatement
@pytest.mark.parametrize("cid", sorted(kc.STAGE_CASES))
def test_stages_of_a_sub_range(dev, cid):
    name, model, shared, s0, ns, params = kc.STAGE_CASES[cid]
    x, m = _tensors(name, dev)
    B, T = x.shape[:2]
    pt = torch.tensor([p + (0.0,) for p in params], dtype=torch.float32, device=dev)
    o = _krig_stages(dev, x, m, model, pt, shared, s0, ns, kc.STAGE_NP, kc.STAGE_CAP, kc.STAGE_MEMBERS, kc.streams_of(B, T))
    r64, r32 = kc.stage_reference(cid, "float64"), kc.stage_reference(cid, "float32")
    f0, nf, R = o["f0"], o["nf"], o["R"]
    assert f0 > 0 and f0 + nf < B * T and not o["status"].any()
    _outside_is_untouched(o)
    inside = slice(f0, f0 + nf)
    for k in CALL_WIDE + ("pred",):
        _within(f"{cid} {k}", o[k][inside].cpu().numpy(), r64[k][inside], r32[k][inside])
    sol = o["sol"].cpu().numpy()                                   # (ns, R + 1, np): u, then K^-1 z of the system's frames
    frames = np.arange(f0, f0 + nf).reshape(ns, R)
    _within(f"{cid} sol u", sol[:, 0], r64["u"][frames[:, 0]], r32["u"][frames[:, 0]])
    _within(f"{cid} sol v", sol[:, 1:], r64["v"][frames], r32["v"][frames])
    alpha = o["alpha"].cpu().numpy()
    for s in range(ns):
        n = int(o["counts"][frames[s, 0]])
        assert not sol[s, :, n:].any() and not alpha[frames[s], n:].any()      # padded unknowns are exactly 0


def test_space_time_stages_of_a_sub_range(dev):
    from p2igan_bench import ops
    name, model, s0, ns, params = kc.ST_STAGE
    x, m = _tensors(name, dev)
    B, T, _, H, W = x.shape
    np_, fcap = kc.STAGE_NP, kc.STAGE_CAP
    pix, z, info = ops.krig_compact(x.reshape(B, T, H, W).contiguous(), m.reshape(B, T, H, W).contiguous(), fcap)
    sites = ops.stkrig_gather_sites(pix, z, info, B, T, np_)
    pt = torch.tensor(params, dtype=torch.float32, device=dev)
    alpha, mean = _sentinel((B, np_), dev), _sentinel((B,), dev)
    pred, var = _sentinel((B * T, fcap), dev), _sentinel((B * T, fcap), dev)
    work = torch.empty(ns * np_ * np_, device=dev, dtype=torch.float32)
    winv = torch.empty_like(work)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    sys = ops.KrigSystems(sites["stpix"], sites["stz"], sites["stinfo"], pt, None, ops.KRIG_MODELS[model], 1, 1, np_, status).chunk(s0, ns)
    ops.stkrig_factor(sys, sites["stt"], work)
    sol = ops.krig_solve(sys, work, alpha, mean)
    ops.krig_invert(work, ns, np_, winv)
    ops.stkrig_loso(sys, ops.stkrig_site_gram(winv, ns, np_), sol, alpha, sites, T, pred, var)
    assert not status.any()
    for t in (alpha, mean):
        assert _is_sentinel(t[:s0]) and _is_sentinel(t[s0 + ns:]) and bool(torch.isfinite(t[s0:s0 + ns]).all())
    counts = info[:B * T].cpu().numpy()
    inside = np.zeros((B * T, fcap), bool)                            # the kernel writes at the points of its samples only
    for f in range(s0 * T, (s0 + ns) * T):
        inside[f, :counts[f]] = True
    got_p, got_v = pred.cpu().numpy(), var.cpu().numpy()
    raw_p, raw_v = pred.view(torch.int32).cpu().numpy(), var.view(torch.int32).cpu().numpy()
    assert (raw_p[~inside] == kc.SENTINEL).all() and (raw_v[~inside] == kc.SENTINEL).all()
    (p64, v64), (p32, v32) = kc.st_reference("float64"), kc.st_reference("float32")
    _within("st LOSO prediction", got_p[inside], p64[inside], p32[inside])
    _within("st LOSO variance", got_v[inside], v64[inside], v32[inside])
    n = int(kc.st_sample_counts(kc.inputs(name)[1])[s0])
    assert not sol.cpu().numpy()[0, :, n:].any() and not alpha[s0, n:].any()


# ---- the descriptor's fields that a stage does not read (include/p2i_hip.h, p2i_krig_systems) may be NULL on the device too
UNREAD = {"krig_factor": ("z", "cand"), "krig_solve": ("pix", "params"), "krig_predict": ("z", "status", "cand"), "krig_variance": ("z",),
          "krig_loo": ("pix", "params"), "krig_cs_weights": ("params",), "krig_cs_predict": (), "stkrig_factor": ("z", "cand"),
          "stkrig_loso": ("pix", "params")}


def _nine_stages(dev, x, m, null):
    """Every stage for systems 1 and 2 of the four per-frame systems (space-time: of four one-frame samples); null: each stage's
    descriptor with its unread pointer fields NULL (and np = 0 for krig_predict, which does not read it)."""
    from p2igan_bench import ops
    B, T, _, H, W = x.shape
    F, HW, M, np_, cap, s0, ns = B * T, H * W, 2, 64, 64, 1, 2
    params = torch.tensor([[0.002, 0.05, 6.0, 1.0]] * F, dtype=torch.float32, device=dev)
    cand = torch.zeros(F, dtype=torch.int32, device=dev)
    zeros = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)      # noqa: E731
    o = {}

    def stage(call, name):
        ch = call.chunk(s0, ns)
        if null:
            for field in UNREAD[name]:
                setattr(ch.c, field, None)
            if name == "krig_predict":
                ch.c.np = 0
        return ch

    def run(call, tag, factor):
        work, winv = torch.empty(ns * np_ * np_, device=dev), torch.empty(ns * np_ * np_, device=dev)
        alpha, mean = zeros(call.F, cap), zeros(call.F)
        factor(stage(call, tag + "krig_factor"), work)
        sol = ops.krig_solve(stage(call, "krig_solve"), work, alpha, mean)
        ops.krig_invert(work, ns, np_, winv)
        o.update({tag + "L": work.view(ns, np_, np_).tril(), tag + "sol": sol, tag + "alpha": alpha, tag + "mean": mean})
        return winv, sol, alpha, mean

    pix, z, info = ops.krig_compact(x.reshape(F, 1, H, W).contiguous(), m.reshape(F, 1, H, W).contiguous(), cap)
    # the dense stages: one system per frame of the (B, T) call
    call = ops.KrigSystems(pix, z, info, params[:B], cand[:B], 0, 1, T, np_, torch.zeros(F, dtype=torch.int32, device=dev))
    winv, sol, alpha, mean = run(call, "", ops.krig_factor)
    o["pred"] = ops.krig_predict(stage(call, "krig_predict"), alpha, mean, H, W, zeros(F, HW))
    o["var"], o["loo_pred"], o["loo_var"], o["ens"] = zeros(F, HW), zeros(F, cap), zeros(F, cap), zeros(F, M, HW)
    ops.krig_variance(stage(call, "krig_variance"), winv, sol, H, W, o["var"])
    ops.krig_loo(stage(call, "krig_loo"), winv, sol, alpha, o["loo_pred"], o["loo_var"])
    amp, _ = ops.krig_cs_spectrum(params[:B], None, 0, H, W, kc.EMBED)
    ops.krig_cs_fields(amp, torch.from_numpy(kc.streams_of(B, T)).reshape(F).to(dev), kc.SEED, T, M, H, W, kc.EMBED, o["ens"])
    o["cs_alpha"], o["cs_mu"] = ops.krig_cs_weights(stage(call, "krig_cs_weights"), winv, sol, o["ens"], M, H, W)
    ops.krig_cs_predict(stage(call, "krig_cs_predict"), o["cs_alpha"], o["cs_mu"], M, H, W, o["ens"])
    # the space-time stages: every frame as a sample of its own
    sites = ops.stkrig_gather_sites(pix, z, info, F, 1, np_)
    st = ops.KrigSystems(sites["stpix"], sites["stz"], sites["stinfo"], params, cand, 0, 1, 1, np_, torch.zeros(F, dtype=torch.int32, device=dev))
    winv, sol, alpha, _ = run(st, "st", lambda ch, L: ops.stkrig_factor(ch, sites["stt"], L))
    o["loso_pred"], o["loso_var"] = zeros(F, cap), zeros(F, cap)
    ops.stkrig_loso(stage(st, "stkrig_loso"), ops.stkrig_site_gram(winv, ns, np_), sol, alpha, sites, 1, o["loso_pred"], o["loso_var"])
    o["status"], o["ststatus"] = call.status, st.status
    return o


def test_unread_descriptor_fields_may_be_null(dev):
    """B = 2, T = 2, 8 x 8, 33 gauges per frame (np = 64: two tiles), fixed exponential parameters, 2 members: each of the nine stages
    with a full descriptor and with the fields it does not read set to NULL gives the same bits."""
    rng = np.random.RandomState(24)
    masks = np.zeros((2, 2, 1, 8, 8), np.float32)
    for f in range(4):
        masks.reshape(4, 64)[f, rng.permutation(64)[:33]] = 1.0
    masked = (rng.rand(2, 2, 1, 8, 8).astype(np.float32) + 0.1) * masks
    x, m = torch.from_numpy(masked).to(dev), torch.from_numpy(masks).to(dev)
    full, null = _nine_stages(dev, x, m, False), _nine_stages(dev, x, m, True)
    assert not full["status"].any() and not full["ststatus"].any()
    assert bool(full["pred"][1:3].any()) and bool(torch.isfinite(full["ens"][1:3]).all()) and bool(torch.isfinite(full["loso_pred"][1:3]).all())
    assert not full["pred"][0].any() and not full["pred"][3].any() and not full["stalpha"][0].any()      # systems 1 and 2 only
    assert sorted(full) == sorted(null)
    for k in full:
        assert _same(full[k], null[k]), (k, "differs once the fields the stage does not read are NULL")


# ---- C: the failed factorisation
def _bad_params(rows, dev):
    return torch.tensor([r + (0.0,) for r in rows], dtype=torch.float32, device=dev)


def _check_failed_and_healthy(what, o, masked, masks, failed, ref=None):
    """failed: per frame of the sub-range, whether its system failed.  The fallback rules on the failed frames, nothing non-finite
    anywhere else, and (ref = (r64, r32) by frame) the healthy frames against the restatement."""
    f0, nf = o["f0"], o["nf"]
    gm = kc.gauge_means(masked, masks).ravel()
    g = {k: o[k][f0:f0 + nf].cpu().numpy() for k in CALL_WIDE + ("pred",)}
    for i in range(nf):
        f, n = f0 + i, int(o["counts"][f0 + i])
        if failed[i]:
            assert abs(g["mean"][i] - gm[f]) <= 1e-6 * abs(gm[f]) and not g["alpha"][i].any(), (what, f)
            assert (g["pred"][i] == g["mean"][i]).all(), (what, f)
            assert np.isnan(g["var"][i]).all() and np.isnan(g["ens"][i]).all(), (what, f)
            for k in ("loo_pred", "loo_var"):
                assert np.isnan(g[k][i, :n]).all() and not g[k][i, n:].any(), (what, f, k)
        else:
            assert all(np.isfinite(g[k][i]).all() for k in g), (what, f)
    if ref is not None:
        ok = np.flatnonzero(~np.asarray(failed, bool))
        for k in g:
            _within(f"{what} healthy {k}", g[k][ok], ref[0][k][f0 + ok], ref[1][k][f0 + ok])


@pytest.mark.parametrize("sub", ["whole", "interior"])
def test_failed_systems_among_healthy_ones(dev, sub):
    """Per-frame systems of one sample, failing in tiles 0, 1 and 2: first, in the middle and last of the call, or of a sub-range."""
    x, m = _tensors("pivot-frames", dev)
    masked, masks = kc.inputs("pivot-frames")
    T = x.shape[1]
    s0, ns = (0, T) if sub == "whole" else kc.PIVOT_SUB
    params, streams = _bad_params([kc.BAD], dev), kc.streams_of(1, T)
    o = _krig_stages(dev, x, m, kc.PIVOT_MODEL, params, False, s0, ns, kc.PIVOT_NP, kc.PIVOT_CAP, 2, streams)
    want = kc.pivot_status()[s0:s0 + ns]
    assert o["status"].cpu().tolist() == want
    _outside_is_untouched(o)
    assert bool(torch.isfinite(o["sol"]).all())                      # the replaced pivot: nothing non-finite was divided by
    ref = tuple(kc.krig_stage_reference(*kc.inputs("pivot-frames-healthy"), kc.PIVOT_MODEL, [kc.BAD], 2, streams[:, kc.pivot_healthy()],
                                        kc.PIVOT_CAP, kc.PIVOT_NP, dt) for dt in ("float64", "float32"))
    healthy = [i for i in kc.pivot_healthy() if s0 <= i < s0 + ns]
    pos = [kc.pivot_healthy().index(i) for i in healthy]            # their frames in the healthy-only input
    spread = tuple({k: np.zeros((T,) + v.shape[1:], v.dtype) for k, v in r.items()} for r in ref)
    for r, sp in zip(ref, spread):
        for k in r:
            sp[k][healthy] = r[k][pos]
    _check_failed_and_healthy(f"pivot-frames {sub}", o, masked, masks, want, spread)
    # the healthy frames alone: bit for bit what they are next to failed ones
    xh, mh = _tensors("pivot-frames-healthy", dev)
    oh = _krig_stages(dev, xh, mh, kc.PIVOT_MODEL, params, False, 0, len(kc.pivot_healthy()), kc.PIVOT_NP, kc.PIVOT_CAP, 2,
                      streams[:, kc.pivot_healthy()])
    assert not oh["status"].any()
    for k in CALL_WIDE + ("pred",):
        assert _same(o[k][healthy], oh[k][pos]), (k, "a failed neighbour leaked into a healthy system")
    assert _same(o["sol"][[i - s0 for i in healthy]], oh["sol"][pos])


def test_failed_sample_next_to_a_healthy_one(dev):
    """One system per sample (R = T, B = 2): sample 0 with the bad parameters fails, sample 1 with benign ones does not."""
    x, m = _tensors("pivot-shared", dev)
    masked, masks = kc.inputs("pivot-shared")
    streams = kc.streams_of(2, 3)
    o = _krig_stages(dev, x, m, kc.PIVOT_MODEL, _bad_params([kc.BAD, kc.BENIGN], dev), True, 0, 2, 64, kc.PIVOT_CAP, 2, streams)
    assert o["status"].cpu().tolist() == [1, 0] and bool(torch.isfinite(o["sol"]).all())
    ref = tuple(kc.krig_stage_reference(masked, masks, kc.PIVOT_MODEL, [kc.BENIGN, kc.BENIGN], 2, streams, kc.PIVOT_CAP, 64, dt)
                for dt in ("float64", "float32"))
    _check_failed_and_healthy("pivot-shared", o, masked, masks, [1, 1, 1, 0, 0, 0], ref)
    means = o["mean"][:3].cpu().tolist()
    assert len(set(means)) == 3                                      # every frame of the failed sample has its own gauge mean
    xh, mh = _tensors("pivot-shared-healthy", dev)
    oh = _krig_stages(dev, xh, mh, kc.PIVOT_MODEL, _bad_params([kc.BENIGN], dev), True, 0, 1, 64, kc.PIVOT_CAP, 2, streams[1:])
    for k in CALL_WIDE + ("pred",):
        assert _same(o[k][3:], oh[k]), (k, "the failed sample leaked into the healthy one")
    assert _same(o["sol"][1:], oh["sol"])


def test_no_model_truth_table(dev):
    """Fitted path (cand given): status 1 with cand >= 0 falls back, status 0 with cand = -1 falls back, status 0 with cand >= 0 does
    not.  Sample 0's fitted parameters are overwritten with the bad ones after the fit."""
    from p2igan_bench import ops
    x, m = _tensors("pivot-table", dev)
    masked, masks = kc.inputs("pivot-table")
    B, T, _, H, W = x.shape
    pix, z, info = ops.krig_compact(x.reshape(B, T, H, W).contiguous(), m.reshape(B, T, H, W).contiguous(), kc.PIVOT_CAP)
    _, _, cand, params = ops.krig_variogram(pix, z, info, B, T, 8, cr.lag_width(H, W, 8), ops.KRIG_MODELS[kc.PIVOT_MODEL])
    assert [c >= 0 for c in cand.cpu().tolist()] == [True, False, True]
    params[0] = torch.tensor(kc.BAD + (0.0,), device=dev)
    streams = kc.streams_of(B, T)
    o = _krig_stages(dev, x, m, kc.PIVOT_MODEL, params, True, 0, B, 64, kc.PIVOT_CAP, 2, streams, cand=cand)
    assert o["status"].cpu().tolist() == [1, 0, 0] and bool(torch.isfinite(o["sol"]).all())
    fitted = [tuple(float(v) for v in row[:3]) for row in params.cpu().numpy()]          # sample 2: the device's own fit, as given
    ref = tuple(kc.krig_stage_reference(masked, masks, kc.PIVOT_MODEL, [fitted[2]] * 3, 2, streams, kc.PIVOT_CAP, 64, dt)
                for dt in ("float64", "float32"))
    _check_failed_and_healthy("pivot-table", o, masked, masks, [1, 1, 1, 1, 0, 0], ref)
    assert bool(o["alpha"][4:].any())                               # the healthy fitted sample has a model


def _one_warning(caplog, number):
    recs = [r for r in caplog.records if r.levelno >= logging.WARNING]
    assert len(recs) == 1 and "non-positive pivot" in recs[0].getMessage() and recs[0].args == (number,), [r.getMessage() for r in recs]
    caplog.clear()


@pytest.mark.parametrize("name,status,each", [("pivot-frames", kc.pivot_status(), 1), ("pivot-shared", [1, 0], 3)])
def test_models_with_a_failed_factorisation(dev, monkeypatch, caplog, name, status, each):
    from p2igan_bench.models import classical
    x, m = _tensors(name, dev)
    masked, masks = kc.inputs(name)
    B, T = x.shape[:2]
    G = _model(dev, name="kriging", max_points=kc.PIVOT_CAP,
               variogram={"model": kc.PIVOT_MODEL, "fit": False, "nugget": 0.0, "psill": kc.PSILL, "range": 4.0})
    # the config rightly refuses a negative nugget; the point here is what happens downstream of a factorisation that fails
    G.fixed = kc.BAD
    failed = np.repeat(np.asarray(status, bool), each)             # per frame
    gm = kc.gauge_means(masked, masks).ravel()
    np_ = kc.round_up(int(kc.counts_of(masks).max()), kc.TILE)
    runs = {}
    for fb in (None, kc.factor_bytes_for(1, np_, False), kc.factor_bytes_for(1, np_, True)):
        if fb is not None:
            monkeypatch.setattr(classical, "_FACTOR_BYTES", fb)
        for entry in ("forward", "forward_uq", "cross_validate", "ensemble2"):
            if fb is not None and (entry == "forward") != (fb == kc.factor_bytes_for(1, np_, False)):
                continue
            caplog.clear()
            with caplog.at_level(logging.WARNING):
                out = _run_entry(G, entry, x, m)
            _one_warning(caplog, sum(status) * each)
            assert out[-1].cpu().tolist() == list(status)
            if fb is None:
                runs[entry] = out
                continue
            for k, (a, b) in enumerate(zip(runs[entry], out)):     # one system per chunk: the same bits
                assert _same(a, b), (name, entry, k)
    pred = runs["forward"][0].reshape(B * T, -1).cpu().numpy()
    assert np.isfinite(pred).all()
    for f in np.flatnonzero(failed):
        assert (pred[f] == pred[f, 0]).all() and abs(pred[f, 0] - gm[f]) <= 1e-6 * abs(gm[f])
    assert _same(runs["forward_uq"][0], runs["forward"][0]) and _same(runs["ensemble2"][0], runs["forward"][0])
    var = runs["forward_uq"][1].reshape(B * T, -1).cpu().numpy()
    ens = runs["ensemble2"][1].reshape(B * T, -1).cpu().numpy()
    for f in range(B * T):
        assert (np.isnan(var[f]).all() and np.isnan(ens[f]).all()) if failed[f] else (np.isfinite(var[f]).all() and np.isfinite(ens[f]).all())
    lp, lv = (t.cpu().numpy() for t in runs["cross_validate"][:2])
    counts = kc.counts_of(masks).ravel()
    for f in range(B * T):
        for a in (lp, lv):
            assert not a[f, counts[f]:].any()
            assert np.isnan(a[f, :counts[f]]).all() if failed[f] else np.isfinite(a[f, :counts[f]]).all()


def test_space_time_model_with_a_failed_factorisation(dev, monkeypatch, caplog):
    from p2igan_bench.models import classical
    x, m = _tensors("pivot-st", dev)
    masked, masks = kc.inputs("pivot-st")
    B, T = x.shape[:2]
    G = _model(dev, name="stkriging", variogram={"model": kc.PIVOT_MODEL, "fit": False, "nugget": 0.0, "psill": kc.PSILL, "range": 4.0,
                                                 "time_scale": kc.PIVOT_KAPPA})
    # the config rightly refuses a negative nugget; the point here is what happens downstream of a factorisation that fails
    G.fixed = kc.BAD + (kc.PIVOT_KAPPA,)
    m64 = (masks != 0).astype(np.float64)
    sample_mean = (masked * m64).sum((1, 2, 3, 4)) / m64.sum((1, 2, 3, 4))
    runs = {}
    for fb in (None, kc.factor_bytes_for(1, 64, False), kc.factor_bytes_for(1, 64, True)):
        if fb is not None:
            monkeypatch.setattr(classical, "_FACTOR_BYTES", fb)
        for entry in ("forward", "cross_validate_sites"):
            if fb is not None and (entry == "forward") != (fb == kc.factor_bytes_for(1, 64, False)):
                continue
            caplog.clear()
            with caplog.at_level(logging.WARNING):
                out = _run_entry(G, entry, x, m)
            _one_warning(caplog, 1)
            assert out[-1].cpu().tolist() == [0, 1, 0]
            if fb is None:
                runs[entry] = out
                continue
            for k, (a, b) in enumerate(zip(runs[entry], out)):
                assert _same(a, b), (entry, k)
    pred = runs["forward"][0].reshape(B, -1).cpu().numpy()
    assert np.isfinite(pred).all() and (pred[1] == pred[1, 0]).all() and abs(pred[1, 0] - sample_mean[1]) <= 1e-6 * sample_mean[1]
    assert pred[0].std() > 0 and pred[2].std() > 0
    lp, lv = (t.reshape(B, T, -1).cpu().numpy() for t in runs["cross_validate_sites"][:2])
    counts = kc.counts_of(masks)
    for b in range(B):
        for t in range(T):
            for a in (lp, lv):
                at = a[b, t, :counts[b, t]]
                assert not a[b, t, counts[b, t]:].any() and (np.isnan(at).all() if b == 1 else np.isfinite(at).all())


# ---- D: a shared set of more than RC = 8 frames
@pytest.mark.parametrize("t", [9, 17])
def test_shared_set_wider_than_a_frame_group(dev, t):
    name = f"wide{t}"
    masked, masks = kc.inputs(name)
    vg = {"model": "exponential", "fit": False, "nugget": 0.002, "psill": 0.05, "range": 6.0}
    r64, r32 = (cr.kriging(masked, masks, vg, dt)[0] for dt in (np.float64, np.float32))
    x, m = _tensors(name, dev)
    G = _model(dev, name="kriging", variogram=vg)
    got = G(x, m).cpu().numpy()
    assert G.last_status.numel() == 1 and int(G.last_status.sum()) == 0          # one system for the t frames
    _within(name, got, r64, r32)
    for f in (kc.RC, t - 1):                                                     # the first frame of group 1 and the last frame
        assert all(not np.array_equal(got[0, f], got[0, g]) for g in range(t) if g != f)
