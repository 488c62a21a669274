"""The differentiable PrimSDF on the MI355X: `primx_primsdf_query_backward` against the float64 autograd of
tests/primsdf_grad_ref.py, `primx_adam_step` against its fp32 numpy restatement bit for bit, the autograd surface of
`PrimSDF(differentiable=True)`, `fit.refine_primitives` next to the restated loop, and the stream-order and footprint cases of the
two entry points.

The backward adds with fp32 atomics, so its sums are not bitwise reproducible; tolerances are 4 x the error of the fp32 CPU
restatement against float64 on the same inputs (the margin covers the other summation order) plus one fp32 ulp of the tensor's
largest magnitude.  Points within DELTA of a kink of the field are dropped before either side runs.

Stream-order cases are REGISTERED here, at import, in the table of tests/test_hip_streams.py (that file stays as it is) and run
here with the same `so.run` call and `called` check as its `test_stream_order`.  The environment fixture `E` is this module's
own: the table's `E` takes two streams from torch's pool for good, and a process that has used one more stream than before binds
the later ones to other hardware queues (there are four) - with this module in front of it, the third-stream control of
tests/test_hip_streams.py found its two streams on ONE queue and reported "ok".  So the one side stream here is created with
hipStreamCreateWithFlags and destroyed when the module is done, which gives its queue share back.  (a) of tests/streamorder.py compares bit for bit,
so these cases are built with at most two contributions per gradient address: two fp32 adds onto zero commute, whichever
arrives first.  Their primitives are disjoint and every primitive holds two points.
"""
import functools

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import primsdf_grad_ref as G
from tests import streamorder as so
from tests import test_hip_streams as TS
from tests.test_hip_streams import called  # noqa: F401  (the stream table's fixture: which primx_* functions a case called)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA = 1e-5
MAX_DROPPED = 0.02
ULP = float(np.finfo(np.float32).eps)
CASES = [(1, 2, 257), (33, 3, 4099), (33, 8, 4099), (1025, 8, 4099)]    # one block plus a lane; ...; across the 1024-primitive chunk


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import _lib, fit, ops, primsdf
    return type("Mods", (), dict(lib=_lib.load(), fit=fit, ops=ops, primsdf=primsdf, check=staticmethod(_lib.check)))


@pytest.fixture(scope="module")
def E(mods):
    """The Env of tests/test_hip_streams.py::E with ONE side stream of this module's own, non-blocking with respect to stream 0
    like torch's pool streams, destroyed at teardown (see the module docstring); `S2` is not needed here."""
    import ctypes
    import os
    from collections import namedtuple

    import topia_xl_amd
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))    # the runtime torch has mapped
    hip.hipStreamCreateWithFlags.argtypes, hip.hipStreamDestroy.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], [ctypes.c_void_p]
    torch.cuda.init()
    with torch.cuda.device(0):
        raw = ctypes.c_void_p()
        assert hip.hipStreamCreateWithFlags(ctypes.byref(raw), 1) == 0 and raw.value                 # 1 = hipStreamNonBlocking
        env = namedtuple("Env", "pkg ops lib S S2 blocker")(topia_xl_amd, mods.ops, mods.lib, torch.cuda.ExternalStream(raw.value), None,
                                                             so.Blocker())
        yield env
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(raw) == 0


# ------------------------------------------------------------------------------------------------ inputs and references
def _inputs(P, S, n, seed=0):
    g = torch.Generator().manual_seed(1000 * P + 10 * S + seed)
    pos = 1.2 * torch.rand(P, 3, generator=g) - 0.6
    scale = 0.15 + 0.2 * torch.rand(P, 1, generator=g)
    feat = 0.5 * torch.randn(P, 6, S ** 3, generator=g)
    feat[:, 1:] += 0.5                                               # tex / mat around 0.5: a share of the outputs clips
    n0 = n // 2
    k = torch.randint(P, (n - n0,), generator=g)
    x = torch.cat([1.8 * torch.rand(n0, 3, generator=g) - 0.9, pos[k] + scale[k] * (2 * torch.rand(n - n0, 3, generator=g) - 1)])
    return x, torch.cat([scale, pos], 1), feat.reshape(P, -1).contiguous(), torch.randn(n, 6, generator=g)


def _reference(x, srt, feat, gout, S):
    """Drop the kinks, then float64 autograd and the tolerance of each gradient from the fp32 restatement's own error."""
    bad = G.kinks(x, srt, feat, S, DELTA)
    keep = ~bad
    x, gout = x[keep].contiguous(), gout[keep].contiguous()
    gs, gf = G.grads(x.double(), srt.double(), feat.double(), gout.double(), S)
    gs32, gf32 = G.grads(x, srt, feat, gout, S)
    tol = {}
    for name, a64, a32 in (("gsrt", gs, gs32), ("gfeat", gf, gf32)):
        top = float(a64.abs().max())
        tol[name] = (4 * float((a32.double() - a64).abs().max()) + ULP * top, top)
    return dict(x=x, srt=srt, feat=feat, gout=gout, gsrt=gs, gfeat=gf, tol=tol, dropped=float(bad.float().mean()), S=S)


@functools.lru_cache(maxsize=None)
def _case(P, S, n):
    return _reference(*_inputs(P, S, n), S)


def _gpu(mods, r, **kw):
    gs, gf = mods.primsdf.query_backward(r["x"].to(DEV), r["srt"].to(DEV), r["feat"].to(DEV), r["gout"].to(DEV), r["S"], **kw)
    return gs, gf


def _compare(tag, r, gs, gf, scale=1.0):
    for name, got in (("gsrt", gs), ("gfeat", gf)):
        if got is None:
            continue
        assert bool(torch.isfinite(got).all()), (tag, name)
        tol, top = r["tol"][name]
        err = float((got.cpu().double() - scale * r[name]).abs().max())
        print(f"{tag} {name}: max-abs error {err:.3e}, tolerance {scale * tol:.3e}, largest entry {scale * top:.3e} "
              f"(error / largest {err / max(scale * top, 1e-300):.2e})")
        assert err <= scale * tol, (tag, name, err, scale * tol)


# ------------------------------------------------------------------------------------------------ 1. kernel vs float64 autograd
@pytest.mark.parametrize("P,S,n", CASES)
def test_backward_matches_float64_autograd(mods, P, S, n):
    r = _case(P, S, n)
    print(f"(P, S, n) = ({P}, {S}, {n}): {100 * r['dropped']:.3f} % of the points dropped as kinks")
    assert r["dropped"] <= MAX_DROPPED
    assert float(r["gsrt"].abs().max()) > 0 and float(r["gfeat"].abs().max()) > 0
    _compare(f"({P}, {S}, {n})", r, *_gpu(mods, r))


# ------------------------------------------------------------------------------------------------ 2. special cases
def test_uncovered_points_leave_the_gradients_exactly_zero(mods):
    x, srt, feat, gout = _inputs(33, 3, 300)
    x = x * 0.01 + 5.0                                                # far from every primitive
    gs, gf = mods.primsdf.query_backward(x.to(DEV), srt.to(DEV), feat.to(DEV), gout.to(DEV), 3)
    assert int((gs != 0).sum()) == 0 and int((gf != 0).sum()) == 0


def test_zero_gout_leaves_the_gradients_exactly_zero(mods):
    r = _case(33, 3, 4099)
    gs, gf = mods.primsdf.query_backward(r["x"].to(DEV), r["srt"].to(DEV), r["feat"].to(DEV), torch.zeros_like(r["gout"]).to(DEV), 3)
    assert int((gs != 0).sum()) == 0 and int((gf != 0).sum()) == 0


def test_negative_scale(mods):
    x, srt, feat, gout = _inputs(33, 3, 1025, seed=1)
    srt[::2, 0] *= -1
    r = _reference(x, srt, feat, gout, 3)
    assert r["dropped"] <= MAX_DROPPED and float(r["gsrt"][::2].abs().max()) > 0
    _compare("negative scale", r, *_gpu(mods, r))


def test_either_gradient_may_be_skipped(mods):
    r = _case(33, 3, 4099)
    gs, gf = _gpu(mods, r, want_feat=False)
    assert gf is None
    _compare("gfeat null", r, gs, None)
    gs, gf = _gpu(mods, r, want_srt=False)
    assert gs is None
    _compare("gsrt null", r, None, gf)


def test_4096_copies_of_one_point_contend_on_eight_voxels(mods):
    x, srt, feat, gout = _inputs(33, 3, 64, seed=2)
    one = _reference(x[40:41], srt, feat, gout[40:41], 3)            # (a point inside a primitive's box)
    assert one["x"].shape[0] == 1 and float(one["gfeat"].abs().max()) > 0
    many = _reference(one["x"].repeat(4096, 1), srt, feat, one["gout"].repeat(4096, 1), 3)
    many["gsrt"], many["gfeat"] = 4096 * one["gsrt"], 4096 * one["gfeat"]          # the restated value: 4096 x the single point's
    _compare("4096 copies", many, *_gpu(mods, many))


# ------------------------------------------------------------------------------------------------ 3. adds, not overwrites
def test_backward_adds_into_prefilled_gradients(mods):
    r = _case(33, 3, 4099)
    pre_s, pre_f = torch.full_like(r["srt"], 0.5), torch.full_like(r["feat"], -0.25)
    gs, gf = _gpu(mods, r, gsrt=pre_s.to(DEV), gfeat=pre_f.to(DEV))
    shifted = dict(r, gsrt=r["gsrt"] + 0.5, gfeat=r["gfeat"] - 0.25)
    shifted["tol"] = {k: (t + ULP * (top + 0.5), top) for k, (t, top) in r["tol"].items()}   # + the rounding of the pre-fill's sum
    _compare("pre-filled", shifted, gs, gf)


# ------------------------------------------------------------------------------------------------ 4. Adam
@pytest.mark.parametrize("n", [1, 257, 33 * (4 + 6 * 27)])
def test_adam_step_is_bit_identical_to_its_fp32_restatement(mods, n):
    g = torch.Generator().manual_seed(n)
    p, m, v = torch.randn(n, generator=g), torch.zeros(n), torch.zeros(n)
    dp, dm, dv = p.to(DEV), m.to(DEV), v.to(DEV)
    p, m, v = p.numpy(), m.numpy(), v.numpy()
    worst = 0
    for t in range(1, 4):
        grad = torch.randn(n, generator=g) * (10.0 ** torch.randint(-4, 2, (n,), generator=g).float())
        dg = grad.to(DEV)
        mods.ops.adam_step(dp, dg, dm, dv, t, lr=1e-2, zero_grad=(t == 2))
        p, m, v = G.adam_step(p, grad.numpy(), m, v, t, lr=1e-2)
        assert torch.equal(dg.cpu(), torch.zeros(n) if t == 2 else grad)                       # the zero-grad flag, and only it
        for name, got, ref in (("param", dp, p), ("m", dm, m), ("v", dv, v)):
            d = np.abs(got.cpu().numpy().view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
            worst = max(worst, int(d.max()))
            assert int(d.max()) == 0, f"step {t}, {name}: {int((d != 0).sum())} of {n} elements differ, by up to {int(d.max())} ulp"
    print(f"adam_step n = {n}: largest difference to the fp32 restatement over 3 steps: {worst} ulp")


# ------------------------------------------------------------------------------------------------ 5. the autograd surface
def _module(mods, r, **kw):
    m = mods.primsdf.PrimSDF(num_prims=r["srt"].shape[0], prim_shape=r["S"], **kw).to(DEV)
    m.srt_param.data, m.feat_param.data = r["srt"].to(DEV), r["feat"].to(DEV)
    return m


def _plain_query(mods, m, x, eval_fill):
    out = torch.empty(x.shape[0], 6, device=DEV)
    mods.check(mods.lib.primx_primsdf_query(x.data_ptr(), m.srt_param.data_ptr(), m.feat_param.data_ptr(), m._linspace(x.device).data_ptr(),
                                            out.data_ptr(), x.shape[0], m.srt_param.shape[0], m.prim_shape, 6, eval_fill,
                                            torch.cuda.current_stream().cuda_stream), "primx_primsdf_query")
    return out


def test_differentiable_module_fills_grad_through_the_kernel(mods):
    r = _case(33, 3, 4099)
    m = _module(mods, r, differentiable=True).train()
    assert m.differentiable is True
    x = r["x"].to(DEV)
    pred = m(x)
    out = torch.cat([pred["sdf"], pred["tex"], pred["mat"]], 1)
    assert out.grad_fn is not None and torch.equal(out.detach(), _plain_query(mods, m, x, 0))
    (out * r["gout"].to(DEV)).sum().backward()
    _compare("autograd", r, m.srt_param.grad, m.feat_param.grad)
    m.zero_grad()
    m.srt_param.requires_grad_(False)                                # only the payload: the srt gradient is skipped
    (m.query(x) * r["gout"].to(DEV)).sum().backward()
    assert m.srt_param.grad is None
    _compare("autograd, payload only", r, None, m.feat_param.grad)
    with pytest.raises(RuntimeError, match="no gradient with respect to"):
        m(x.clone().requires_grad_(True))


def test_every_other_state_runs_the_present_path(mods):
    r = _case(33, 3, 4099)
    x = r["x"].to(DEV)
    default = _module(mods, r)
    assert default.differentiable is False
    for training in (True, False):
        want = _plain_query(mods, default, x, 0 if training else 1)
        for m in (default.train(training), _module(mods, r, differentiable=True).train(training)):
            if m.differentiable and training:
                with torch.no_grad():
                    out = m.query(x)                                  # grad mode off
                assert out.grad_fn is None and torch.equal(out, want)
                m.requires_grad_(False)                               # no parameter requires grad
            out = m.query(x)
            assert out.grad_fn is None and not out.requires_grad and torch.equal(out, want)
    out = default.train().query(x.clone().requires_grad_(True))       # not differentiable: x.requires_grad is ignored, as before
    assert out.grad_fn is None


# ------------------------------------------------------------------------------------------------ 6. refinement
def _icosphere(mods, **kw):
    from tests import meshfield_numpy as MF
    v, f = MF.icosphere(1)
    attr = torch.as_tensor(MF.affine_attr(v)).float().to(DEV)
    mesh = (torch.as_tensor(v).float().to(DEV), torch.as_tensor(f).int().to(DEV), attr[:, :3].contiguous(), attr[:, 3].contiguous(),
            attr[:, 4].contiguous())
    return mods.fit.mesh_to_primitives(mesh, num_prims=33, prim_shape=3, candidates=300, **kw)


def test_refinement_follows_the_float64_restated_loop(mods):
    """The GPU loop next to the restated one: same mesh, same seeded point set, the targets of the GPU's own mesh field.
    Recorded on the MI355X: see DESIGN.md "Refinement"."""
    recon, info = _icosphere(mods)
    field = mods.fit.MeshField(info["v"], info["f"], info["attr"])
    out, rinfo = mods.fit.refine_primitives(recon, field, 20, samples_per_prim=64, refine_srt=True)          # payload and srt: both Adam launches
    pts, target = rinfo["points"].cpu(), rinfo["target"].cpu()
    assert torch.equal(pts, G.refine_points(recon[:, :4].cpu(), 64, 0))
    _, l64 = G.refine(recon.cpu(), target, pts, 20, 3, dtype=torch.float64)
    _, l32 = G.refine(recon.cpu(), target, pts, 20, 3, dtype=torch.float32)
    assert l64[-1] < l64[0]                                           # the restated loss falls
    drift = max(abs(a - b) / b for a, b in zip(l32, l64))
    got = max(abs(a - b) / b for a, b in zip(rinfo["loss"], l64))
    print(f"refinement, 20 steps: loss {l64[0]:.4e} -> {l64[-1]:.4e}; fp32 restatement drift {drift:.3e}, GPU {got:.3e} (relative, worst step)")
    assert len(rinfo["loss"]) == 20 and got <= 4 * drift, (got, drift)
    assert bool(torch.isfinite(out).all()) and out.shape == recon.shape
    assert not torch.equal(out[:, :4], recon[:, :4]) and not torch.equal(out[:, 4:], recon[:, 4:])
    frozen, _ = mods.fit.refine_primitives(recon, field, 2, samples_per_prim=8)                        # the default leaves srt alone
    assert torch.equal(frozen[:, :4], recon[:, :4]) and not torch.equal(frozen[:, 4:], recon[:, 4:])


def test_refine_zero_is_the_initialisation_bit_for_bit(mods):
    plain, _ = _icosphere(mods)
    zero, info0 = _icosphere(mods, refine=0)
    three, info3 = _icosphere(mods, refine=3)
    assert torch.equal(plain, zero) and "refine" not in info0
    assert len(info3["refine"]["loss"]) == 3 and not torch.equal(three, plain)
    m = mods.primsdf.PrimSDF.from_mesh((info0["v"], info0["f"], info0["attr"][:, :3].contiguous(), info0["attr"][:, 3].contiguous(),
                                        info0["attr"][:, 4].contiguous()), num_prims=33, prim_shape=3, candidates=300, normalize=False,
                                       refine=3)
    assert not m.training and tuple(m.feat_param.shape) == (33, 6 * 27)


# ------------------------------------------------------------------------------------------------ 7. stream order and footprint
def _disjoint(P, cells, scale, k, S):
    """P primitives on a cells^3 lattice of [-0.8, 0.8]^3 that do not touch, two points inside each: every gradient address receives
    at most two contributions, so the atomic sums are the same bits in any arrival order."""
    g = torch.Generator().manual_seed(31 * P + k)
    idx = torch.randperm(cells ** 3, generator=g)[:P]
    step = 1.6 / cells
    pos = torch.stack([idx % cells, (idx // cells) % cells, idx // cells ** 2], 1).float() * step - 0.8 + 0.5 * step
    assert scale < 0.5 * step
    srt = torch.cat([torch.full((P, 1), scale), pos], 1)
    feat = 0.5 * torch.randn(P, 6 * S ** 3, generator=g) + 0.3
    x = (pos[:, None, :] + scale * (1.8 * torch.rand(P, 2, 3, generator=g) - 0.9)).reshape(-1, 3)
    return srt, feat, x, torch.randn(2 * P, 6, generator=g)


@TS.case("primsdf_query_backward", ["primx_primsdf_query_backward"])
def _stream_backward(E, dtype):
    from topia_xl_amd import primsdf

    def make(k):
        srt, feat, x, gout = _disjoint(1025, 11, 0.06, k, 8)         # two LDS chunks of primitives
        return {"srt": srt.to(DEV), "feat": feat.to(DEV), "x": x.to(DEV).contiguous(), "gout": gout.to(DEV)}

    def call(ctx, i, probe):
        return list(primsdf.query_backward(i["x"], i["srt"], i["feat"], i["gout"], 8))
    return make, call, None


@TS.case("adam_step", ["primx_adam_step"])
def _stream_adam(E, dtype):
    def make(k):
        return {"p": TS.R(k, "adam.p", 70001), "g": TS.R(k, "adam.g", 70001, scale=0.1), "m": TS.R(k, "adam.m", 70001, scale=0.01),
                "v": TS.R(k, "adam.v", 70001, scale=0.01).abs()}

    def call(ctx, i, probe):
        E.ops.adam_step(i["p"], i["g"], i["m"], i["v"], 3, lr=1e-2, zero_grad=True)
        return [i["p"], i["g"], i["m"], i["v"]]
    return make, call, None


@TS.case("refine_primitives", ["primx_primsdf_query", "primx_primsdf_query_backward", "primx_adam_step", "primx_mesh_field_query"])
def _stream_refine(E, dtype):
    from tests import meshfield_numpy as MF
    from topia_xl_amd import fit
    v, f = MF.icosphere(1)
    attr = MF.affine_attr(v)

    def make(k):
        srt, feat, _, _ = _disjoint(33, 4, 0.15, k, 3)
        return {"recon": torch.cat([srt, feat], 1).to(DEV).contiguous(), "v": TS._dev(v, TS.F32) * (1.0 + 0.2 * k), "f": TS._dev(f, torch.int32),
                "attr": TS._dev(attr, TS.F32)}

    def call(ctx, i, probe):
        out, info = fit.refine_primitives(i["recon"], fit.MeshField(i["v"], i["f"], i["attr"]), 3, samples_per_prim=2, refine_srt=True)
        return [out, info["target"], info["loss"]]
    return make, call, None


STREAM_CASES = ("primsdf_query_backward", "adam_step", "refine_primitives")
STREAM_MUST_SYNC = {
    "refine_primitives": "the targets come from MeshField.query, whose C host reads its index check back (MUST_SYNC of mesh_field_query), "
                         "and the losses are read back once after the last step; the steps themselves do not synchronise",
}


@pytest.mark.parametrize("name", STREAM_CASES)
def test_stream_order_of_the_refinement_entry_points(E, called, name):  # noqa: F811  (`called` is the imported fixture)
    """The body of tests/test_hip_streams.py::test_stream_order for the cases registered above."""
    c = TS.CASES[name]
    make, call, setup = c.build(E, None)
    rep = so.run(name, make, call, E.S, E.blocker, setup=setup, must_sync=name in STREAM_MUST_SYNC)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{name} declares entry points it did not call: {missing}"


def test_footprint_of_the_refinement_entry_points(mods):
    """Both entry points inside footprint.guarded, under both fills: nothing is written outside gsrt / gfeat and the four Adam
    arrays (their guards, and the guards and contents of every const operand, are intact), and the results do not depend on
    the fill.  The backward's sums are atomic, so the fills are compared within the tolerance of the reference, not bit for bit."""
    r = _case(1025, 8, 4099)
    n = 33 * (4 + 6 * 27)
    p0, g0 = torch.randn(n, generator=torch.Generator().manual_seed(3)), torch.randn(n, generator=torch.Generator().manual_seed(4))
    pr, mr, vr = G.adam_step(p0.numpy(), g0.numpy(), np.zeros(n, np.float32), np.zeros(n, np.float32), 1)
    for fill in fp.FILLS:
        with fp.guarded(fill) as g:
            x, srt, feat, gout = (g.guard_input(r[k].to(DEV), k).t for k in ("x", "srt", "feat", "gout"))
            gs, gf = mods.primsdf.query_backward(x, srt, feat, gout, 8)                     # (zeros_like inside the package: guarded)
            own = g.guard_input(torch.zeros(1025, 4, device=DEV), "gsrt", const=False).t    # a caller's own accumulator
            mods.primsdf.query_backward(x, srt, feat, gout, 8, gsrt=own, want_feat=False)
            p, gr, m, v = (g.guard_input(t.to(DEV), k, const=False).t for k, t in (("p", p0), ("g", g0), ("m", torch.zeros(n)), ("v", torch.zeros(n))))
            mods.ops.adam_step(p, gr, m, v, 1, zero_grad=True)
            assert len(g.records) >= 11 and not g.bypassed
        _compare(f"fill {fill:#04x}", r, gs, gf)
        _compare(f"fill {fill:#04x}, own gsrt", r, own, None)
        assert np.array_equal(p.cpu().numpy(), pr) and np.array_equal(m.cpu().numpy(), mr) and np.array_equal(v.cpu().numpy(), vr)
        assert int((gr != 0).sum()) == 0
