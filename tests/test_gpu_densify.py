"""GPU: densify-and-prune (gsr_densify_plan / gsr_densify_apply, csrc/densify.hip;
gaussiansplattingviewer_amd.densify) against the numpy restatement of tests/densify_reference.py:
BIT FOR BIT for the counts, source_index, every parameter word except the children's xyz, both
moments and the fresh statistics; the children's xyz within 8 x the float32 spread measured on
the CPU (densify_reference.SPREAD, in the units stated there) of the float64 positions.

   1 P in {1, 2, 63, 64, 65, 255, 256, 257, 1000, 1029} x both scale spaces x the class patterns
     (all kept, all cloned, all split, all pruned, a random mix with denom == 0 rows, long runs,
     rows AT every threshold and one float beside it), the radius test on, and off for the mix;
     the 3DGS six (f_rest M = 45) and an M = 17 tensor without moments; every buffer at a pointer
     that is 4-byte aligned only, between guard words; NaN in every word the apply must not read.
     A scan block is 256 rows: P = 1000 is three blocks and a partial one, 1029 four and a partial
   2 P = 66000: 258 scan blocks, so the finishing block's loop over the block sums runs twice
   3 the routes (`_C`, ctypes, densify_and_prune) and a second stream give the same bits; the
     same seed twice gives the same bits, another seed changes the children's xyz only
   4 densify_and_prune: the optimizer's groups rebound, torch's state keys, `step` kept, moments
     [P', M]; SparseGaussianAdam.step runs on them; more than 8 groups; P' = 0; the refusals that
     need a device
   5 output element indices past 2^31: the four roles and one wide tensor without moments
"""
import numpy as np
import pytest
import torch

import densify_reference as D
import optimizer_reference as R
from gaussiansplattingviewer_amd import SparseGaussianAdam, _lib, densify, densify_and_prune

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0x7FC0BEEF  # a NaN no arithmetic produces
PAD = 16
SEED = 0x9E3779B97F4A7C15  # both key words in use


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.uint32 else a


class Guarded:
    """A device buffer holding `host` between guard words, the data at a pointer that is 4-byte
    aligned only (lead = PAD + 1)."""

    def __init__(self, host, gpu, lead=PAD + 1):
        host = np.ascontiguousarray(host)
        assert host.dtype.itemsize == 4
        full = np.full(lead + host.size + PAD, GUARD, np.uint32)
        full[lead:lead + host.size] = host.reshape(-1).view(np.uint32)
        self.buf = torch.as_tensor(full.view(np.int32)).to(gpu)
        kind = torch.float32 if host.dtype == F else torch.int32
        self.t = self.buf[lead:lead + host.size].view(kind).view(host.shape)
        self.lead, self.n = lead, host.size

    def check(self):
        """The guards are intact -> the data's bits."""
        full = self.buf.cpu().numpy().view(np.uint32)
        assert (full[:self.lead] == GUARD).all() and (full[self.lead + self.n:] == GUARD).all()
        return full[self.lead:self.lead + self.n]


def unwritten(shape, dtype=F):
    return np.full(shape, GUARD, np.uint32).view(dtype)


def upload(sc, gpu):
    dev = dict(groups=[{k: None if g[k] is None else Guarded(g[k], gpu) for k in "pmv"}
                       for g in sc["groups"]],
               accum=Guarded(sc["grad_accum"], gpu), denom=Guarded(sc["denom"], gpu),
               radii=None if sc["max_radii"] is None else Guarded(sc["max_radii"], gpu))
    by_role = {g["role"]: d for g, d in zip(sc["groups"], dev["groups"]) if g["role"]}
    dev["inputs"] = lambda seed: densify.DensifyInputs(  # noqa: E731
        dev["accum"].t, dev["denom"].t, None if dev["radii"] is None else dev["radii"].t,
        by_role["scaling"]["p"].t, by_role["opacity"]["p"].t,
        tuple(float(v) for v in sc["thresholds"]), sc["radius_threshold"],
        _lib.GSR_SCALE_LOG if sc["log_space"] else _lib.GSR_SCALE_LINEAR, seed)
    return dev


def run_gpu(sc, dev, gpu, seed=SEED, route="ctypes"):
    """plan -> counts -> guarded outputs -> apply.  -> (counts, out groups, source_index)."""
    P = len(sc["grad_accum"])
    inp = dev["inputs"](seed)
    ws = Guarded(unwritten(densify.workspace_words(P), np.int32), gpu)
    counts = Guarded(unwritten(4, np.int32), gpu)
    densify.plan(inp, ws.t, counts.t, route)
    n = counts.check().view(np.int32)
    ws.check()
    P_out = int(n[0] + n[1] + 2 * n[2])
    out = [{k: None if g[k] is None else Guarded(unwritten((P_out,) + g[k].shape[1:]), gpu)
            for k in "pmv"} for g in sc["groups"]]
    index = Guarded(unwritten(P_out, np.int32), gpu)
    as_tuple = lambda d: (d["p"].t, None if d["m"] is None else d["m"].t,  # noqa: E731
                          None if d["v"] is None else d["v"].t)
    densify.apply(inp, [g["role"] for g in sc["groups"]], [as_tuple(d) for d in dev["groups"]],
                  [as_tuple(d) for d in out], ws.t, index.t, route)
    return tuple(int(v) for v in n), out, index


def compare(sc, dev, want, got, what):
    """Everything but the children's xyz bit for bit; those within 8 x SPREAD x scale.  The
    sources keep their bits (NaN poison included).  -> the children's xyz bits."""
    counts, out, index = got
    assert counts == want["counts"], what
    np.testing.assert_array_equal(index.check().view(np.int32), want["source_index"], err_msg=what)
    children = want["children"]
    xyz_bits = None
    for g, d, w in zip(sc["groups"], out, want["groups"]):
        p = d["p"].check().reshape(w["p"].shape)
        ref = _bits(w["p"])
        if g["role"] == "xyz":
            xyz_bits = p[children].copy()
            pos = xyz_bits.view(F).astype(np.float64)
            err = np.abs(pos - want["xyz64"]).max(1) if len(pos) else np.zeros(0)
            assert (err <= 8 * D.SPREAD * want["scale"]).all(), \
                f"{what}: child xyz off by {(err / want['scale']).max():.3g} x scale"
            p, ref = np.delete(p, children, 0), np.delete(ref, children, 0)
        np.testing.assert_array_equal(p, ref, err_msg=f"{what}: {g['name']} param")
        for k in "mv":
            if w[k] is None:
                assert d[k] is None
            else:
                np.testing.assert_array_equal(d[k].check(), _bits(w[k]).reshape(-1),
                                              err_msg=f"{what}: {g['name']} {k}")
    for g, d in zip(sc["groups"], dev["groups"]):
        for k in "pmv":
            if g[k] is not None:
                np.testing.assert_array_equal(d[k].check(), _bits(g[k]).reshape(-1))
    np.testing.assert_array_equal(dev["accum"].check(), _bits(sc["grad_accum"]))
    np.testing.assert_array_equal(dev["denom"].check(), _bits(sc["denom"]))
    assert all(np.isfinite(w["p"]).all() for w in want["groups"])
    return xyz_bits


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_space", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1029])
def test_against_the_restatement(P, log_space, gpu):
    rng = np.random.default_rng(100 * P + log_space)
    seen = np.zeros(4, np.int64)
    for pattern, radius_on in [(p, True) for p in sorted(D.PATTERNS)] + [("mix", False),
                                                                        ("edges", False)]:
        sc = D.make_scene(P, rng, log_space, pattern, radius_on=radius_on)
        want = D.run(sc, SEED)
        dev = upload(sc, gpu)
        compare(sc, dev, want, run_gpu(sc, dev, gpu), f"P {P} {pattern} radius {radius_on}")
        seen += want["counts"]
        if pattern in ("keep", "clone", "split", "prune"):
            nk, nc, ns, nr = want["counts"]
            assert dict(keep=nk == P and nc == 0, clone=nk == P and nc == P, split=ns == P,
                        prune=nr == P and nk + nc + ns == 0)[pattern]
        if pattern == "edges" and P >= 8:
            # rows 0..7: avg == t hot clone; smax == t clone; o == t stays; r == t stays; avg one
            # below cold; smax one above split; o one below goes; r == t + 1 goes (radius on)
            src = want["source_index"]
            nk, nc, ns, _ = want["counts"]
            kept, cloned, split = src[:nk], src[nk:nk + nc], src[nk + nc:nk + nc + ns]
            assert {0, 1, 2, 3, 4} <= set(kept) and {0, 1} <= set(cloned) and 5 in split
            assert 4 not in cloned and 6 not in src and (7 in kept) != radius_on
    assert (seen > 0).all()


# ---- 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["mix", "runs"])
def test_more_scan_blocks_than_one_finishing_pass(pattern, gpu):
    P = 66000
    assert (P + 255) // 256 > 256
    sc = D.make_scene(P, np.random.default_rng(66), True, pattern, groups=D.ROLES_ONLY)
    want = D.run(sc, SEED)
    assert min(want["counts"]) > 256
    dev = upload(sc, gpu)
    compare(sc, dev, want, run_gpu(sc, dev, gpu), f"P {P} {pattern}")


# ---- 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_space", [False, True], ids=["linear", "log"])
def test_routes_streams_and_seeds(log_space, gpu):
    P = 777
    sc = D.make_scene(P, np.random.default_rng(3), log_space, "mix")
    want = D.run(sc, SEED)
    dev = upload(sc, gpu)
    first = compare(sc, dev, want, run_gpu(sc, dev, gpu, route="ctypes"), "ctypes")
    for route in ("_C", "ctypes", None):
        again = compare(sc, dev, want, run_gpu(sc, dev, gpu, route=route), f"route {route}")
        np.testing.assert_array_equal(again, first, err_msg=f"route {route}: child xyz")
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        got = run_gpu(sc, dev, gpu, route="_C")
    side.synchronize()
    np.testing.assert_array_equal(compare(sc, dev, want, got, "second stream"), first)
    # another seed: compare() holds everything but the children's xyz to the same bits
    other = D.run(sc, SEED + 1)
    moved = compare(sc, dev, other, run_gpu(sc, dev, gpu, seed=SEED + 1), "another seed")
    assert (moved != first).any(1).all()
    high = compare(sc, dev, D.run(sc, SEED ^ (1 << 63)), run_gpu(sc, dev, gpu, SEED ^ (1 << 63)),
                   "the seed's high word")
    assert (high != first).any(1).all()


# ---- 4 ------------------------------------------------------------------------------------------
WRAPPER = dict(max_grad=D.LINEAR[0], min_opacity=D.LINEAR[2], extent=20.0, percent_dense=0.0125)
RENAMED = dict(xyz="means3D", scaling="scales", rotation="rotations", opacity="opacities")


def make_optimizer(sc, gpu, names=None):
    names = names or {}
    params = {names.get(g["name"], g["name"]): torch.nn.Parameter(torch.as_tensor(g["p"]).to(gpu))
              for g in sc["groups"]}
    opt = SparseGaussianAdam([{"params": [p], "lr": 1e-3 * (i + 1), "name": n}
                              for i, (n, p) in enumerate(params.items())], lr=0.0, eps=1e-15)
    for g, p in zip(sc["groups"], params.values()):
        if g["m"] is not None:
            opt.state[p] = dict(step=torch.tensor(5.0), exp_avg=torch.as_tensor(g["m"]).to(gpu),
                                exp_avg_sq=torch.as_tensor(g["v"]).to(gpu))
    return opt, params


@pytest.mark.parametrize("log_space, screen", [(False, 20), (True, 20.5), (True, None)])
def test_densify_and_prune(log_space, screen, gpu):
    P = 600
    sc = D.make_scene(P, np.random.default_rng(4), log_space, "mix", radius_on=screen is not None,
                      poison=screen is not None)
    if screen is None:  # upstream's behaviour: neither the screen-size nor the world-size test
        sc["thresholds"] = sc["thresholds"][:3] + (F(np.inf),)
    stored = densify.stored_thresholds(WRAPPER["max_grad"], WRAPPER["min_opacity"],
                                       WRAPPER["extent"], screen, WRAPPER["percent_dense"],
                                       activated=not log_space)
    assert stored == (tuple(float(v) for v in sc["thresholds"]), sc["radius_threshold"])
    want = D.run(sc, 12345)
    names = RENAMED if log_space else None
    opt, params = make_optimizer(sc, gpu, names)
    accum = torch.as_tensor(sc["grad_accum"]).to(gpu).reshape(P, 1)
    denom = torch.as_tensor(sc["denom"]).to(gpu).reshape(P, 1)
    radii = None if sc["max_radii"] is None else torch.as_tensor(sc["max_radii"]).to(gpu)
    r = densify_and_prune(opt, accum, denom, radii, max_screen_size=screen, seed=12345,
                          roles=names, activated=not log_space, **WRAPPER)
    nk, nc, ns, nr = want["counts"]
    P_out = nk + nc + 2 * ns
    assert tuple(r.counts) == want["counts"] and r.counts.total == P_out
    np.testing.assert_array_equal(r.source_index.cpu().numpy(), want["source_index"])
    assert r.grad_accum.shape == (P_out, 1) and r.denom.shape == (P_out, 1)
    assert r.grad_accum.dtype == torch.float32 and not r.grad_accum.any() and not r.denom.any()
    if radii is None:
        assert r.max_radii2D is None
    else:
        assert r.max_radii2D.shape == (P_out,) and r.max_radii2D.dtype == torch.int32
        assert not r.max_radii2D.any()
    assert list(r.params) == list(params)
    children = want["children"]
    for group, g, w, (name, old) in zip(opt.param_groups, sc["groups"], want["groups"],
                                        params.items()):
        new = group["params"][0]
        assert new is r.params[name] and isinstance(new, torch.nn.Parameter) and new.requires_grad
        assert new.shape == (P_out,) + old.shape[1:] and old not in opt.state
        got, ref = _bits(new), _bits(w["p"])
        if g["role"] == "xyz":
            err = np.abs(got[children].view(F).astype(np.float64) - want["xyz64"]).max(1)
            assert (err <= 8 * D.SPREAD * want["scale"]).all()
            got, ref = np.delete(got, children, 0), np.delete(ref, children, 0)
        np.testing.assert_array_equal(got, ref, err_msg=name)
        if g["m"] is None:
            assert new not in opt.state
            continue
        st = opt.state[new]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 5.0
        assert st["exp_avg"].shape == new.shape and st["exp_avg_sq"].shape == new.shape
        np.testing.assert_array_equal(_bits(st["exp_avg"]), _bits(w["m"]), err_msg=name)
        np.testing.assert_array_equal(_bits(st["exp_avg_sq"]), _bits(w["v"]), err_msg=name)
    # the optimizer steps on the rebound groups: one group checked against the restatement
    rng = np.random.default_rng(9)
    grads = {}
    for group, g in zip(opt.param_groups, sc["groups"]):
        if g["m"] is not None:
            grads[group["name"]] = R.gradients(rng, tuple(group["params"][0].shape))
            group["params"][0].grad = torch.as_tensor(grads[group["name"]]).to(gpu)
    opt.step(None, P_out)
    group, w = opt.param_groups[1], want["groups"][1]
    p1, m1, v1 = R.adam_step(w["p"], grads[group["name"]], w["m"], w["v"], group["lr"], 1e-15,
                             0.9, 0.999)
    st = opt.state[group["params"][0]]
    assert float(st["step"]) == 6.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
    np.testing.assert_array_equal(_bits(group["params"][0]), _bits(p1))
    np.testing.assert_array_equal(_bits(st["exp_avg"]), _bits(m1))
    np.testing.assert_array_equal(_bits(st["exp_avg_sq"]), _bits(v1))
    assert len(opt.state) == sum(g["m"] is not None for g in sc["groups"])


def test_densify_and_prune_on_more_than_eight_groups_and_on_nothing(gpu):
    P = 300
    more = D.GROUPS + tuple((f"more{i}", i + 1, None, i % 2 == 0) for i in range(4))
    sc = D.make_scene(P, np.random.default_rng(5), False, "mix", groups=more, poison=False)
    assert len(sc["groups"]) == 11
    want = D.run(sc, 1)
    opt, params = make_optimizer(sc, gpu)
    kw = dict(max_screen_size=20, seed=1, activated=True, **WRAPPER)
    z = lambda k: torch.as_tensor(sc[k]).to(gpu)  # noqa: E731
    r = densify_and_prune(opt, z("grad_accum"), z("denom"), z("max_radii"), **kw)
    assert tuple(r.counts) == want["counts"]
    for g, w in zip(sc["groups"], want["groups"]):
        if g["role"] != "xyz":
            np.testing.assert_array_equal(_bits(r.params[g["name"]]), _bits(w["p"]),
                                          err_msg=g["name"])
    # every row pruned: P' = 0, empty tensors, the state's moments empty too
    n = r.counts.total
    gone = densify_and_prune(opt, torch.zeros(n, device=gpu), torch.ones(n, device=gpu), None,
                             max_grad=1.0, min_opacity=1.0, extent=20.0, seed=1, activated=True)
    assert tuple(gone.counts) == (0, 0, 0, n) and gone.source_index.numel() == 0
    assert all(p.shape[0] == 0 for p in gone.params.values())
    assert opt.state[gone.params["xyz"]]["exp_avg"].shape == (0, 3)
    # and P = 0 in: nothing to do
    again = densify_and_prune(opt, torch.zeros(0, device=gpu), torch.zeros(0, device=gpu), None,
                              max_grad=1.0, min_opacity=0.5, extent=20.0, seed=1, activated=True)
    assert tuple(again.counts) == (0, 0, 0, 0)
    # refusals that need a device
    opt, params = make_optimizer(sc, gpu)
    a, d = z("grad_accum"), z("denom")
    with pytest.raises(ValueError, match="grad_accum must hold 300"):
        densify_and_prune(opt, a[:-1], d, **kw)
    with pytest.raises(ValueError, match="denom must hold 300"):
        densify_and_prune(opt, a, d.double(), **kw)
    with pytest.raises(ValueError, match="max_radii2D must hold 300"):
        densify_and_prune(opt, a, d, z("max_radii").long(), **kw)
    with pytest.raises(ValueError, match="HIP device"):
        densify_and_prune(opt, a.cpu(), d, **kw)
    with pytest.raises(ValueError, match="must be contiguous"):
        densify_and_prune(opt, torch.stack([a, a], 1)[:, 0], d, **kw)
    opt.param_groups[2]["params"][0] = torch.nn.Parameter(torch.zeros(P + 1, 45, device=gpu))
    with pytest.raises(ValueError, match="expected 300 rows"):
        densify_and_prune(opt, a, d, **kw)
    opt.param_groups[2]["params"][0] = torch.nn.Parameter(torch.zeros(45, P, device=gpu).t())
    with pytest.raises(ValueError, match="contiguous float32"):
        densify_and_prune(opt, a, d, **kw)
    opt.param_groups[2]["params"][0] = params["f_rest"]
    opt.param_groups[0]["params"][0] = torch.nn.Parameter(torch.zeros(P, 4, device=gpu))
    with pytest.raises(ValueError, match="expected 3"):
        densify_and_prune(opt, a, d, **kw)


# ---- 5 ------------------------------------------------------------------------------------------
def test_output_indices_past_two_to_the_31(gpu):
    """The four roles and one tensor of M = 2^31 / 72 + 12345 floats without moments; every one of
    the 40 rows is kept and cloned, so the last rows of the 80 written lie past word 2^31.  The
    wide tensor (4.8 GB in, 9.5 GB out) never leaves the device: it is compared there."""
    P, M = 40, (1 << 31) // 72 + 12345
    assert 72 * M > (1 << 31) and M > 1024
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 32 * 2 ** 30:
        pytest.skip(f"needs 32 GiB of free device memory, {free / 2 ** 30:.0f} GiB are free")
    sc = D.make_scene(P, np.random.default_rng(31), True, "clone", groups=D.ROLES_ONLY)
    want = D.run(sc, SEED)
    assert want["counts"] == (P, P, 0, 0)
    dev = upload(sc, gpu)
    inp = dev["inputs"](SEED)
    wide = torch.randint(-2 ** 31, 2 ** 31 - 1, (P, M), dtype=torch.int32, device=gpu)
    out_wide = torch.full((2 * P, M), 0x7FC0BEEF, dtype=torch.int32, device=gpu)
    ws = torch.empty(densify.workspace_words(P), dtype=torch.int32, device=gpu)
    counts = torch.empty(4, dtype=torch.int32, device=gpu)
    densify.plan(inp, ws, counts, "ctypes")
    assert tuple(counts.tolist()) == want["counts"]
    out = [{k: Guarded(unwritten((2 * P,) + g[k].shape[1:]), gpu) for k in "pmv"}
           for g in sc["groups"]]
    index = Guarded(unwritten(2 * P, np.int32), gpu)
    src = [(d["p"].t, d["m"].t, d["v"].t) for d in dev["groups"]]
    dst = [(d["p"].t, d["m"].t, d["v"].t) for d in out]
    densify.apply(inp, [g["role"] for g in sc["groups"]] + [None],
                  src + [(wide.view(torch.float32), None, None)],
                  dst + [(out_wide.view(torch.float32), None, None)], ws, index.t, "ctypes")
    np.testing.assert_array_equal(index.check().view(np.int32), want["source_index"])
    for d, w in zip(out, want["groups"]):
        np.testing.assert_array_equal(d["p"].check(), _bits(w["p"]).reshape(-1))
        np.testing.assert_array_equal(d["m"].check(), _bits(w["m"]).reshape(-1))
    for half in (out_wide[:P], out_wide[P:]):
        assert torch.equal(half, wide)
    del wide, out_wide, half
    torch.cuda.empty_cache()
