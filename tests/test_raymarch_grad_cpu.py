"""tests/raymarch_grad_ref.py and the differentiable marcher's Python surface without a GPU: the restatement against the oracle's
forward and against the gradients of the reference's own PyTorch loop (tests/golden/raymarch_grad.npz), the decision margins of
the GPU scenes of tests/test_hip_raymarch_grad.py, the training-time ray subsample, the closure of the stream-order table once that
module's case is registered, and the ABI."""
import os

import numpy as np
import pytest
import torch

from oracle import raymarch_ref
from tests import raymarch_grad_ref as G
from tests import raymarch_replay as rr
from tests import raymarch_scenes as sc
from tests import test_hip_raymarch_grad as TG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ (a) restatement vs the reference
def test_restated_forward_matches_the_oracle_loop():
    """The dt = 0.02 scene of tests/test_raymarch_contract.py::test_replay_matches_oracle_loop, held the same way: within the
    replay's own per-pixel bound (the oracle is fp32 and tests |y| < 1 without a band)."""
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(seed=3, N=1, K=24, H=20, W=18, dist=3.0)
    _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, 20, 18)
    with torch.no_grad():
        img, info = G.march(rp, rd, tm, 0.02, pos.double(), rot.double(), scale.double(), tpl.double(), 8.0, 8.0)
    ex, bd, _ = rr.replay(rp, rd, tm, 0.02, pos, rot, scale, tpl, 8.0, 8.0)
    ref = raymarch_ref.raymarch(rp, rd, tm, 0.02, pos, rot, scale, tpl, 8.0, 8.0).double()
    assert float(ref[..., 3].max()) > 0.99 and info["saturated"] > 0
    print(f"restatement vs replay {float((img - ex).abs().max()):.3e}, vs oracle {float((img - ref).abs().max()):.3e}")
    # the replay evaluates the same samples at the fp32-rounded y, the restatement at the float64 y: inside the replay's bound too
    assert bool(((img - ex).abs() <= bd).all())
    assert bool(((img - ref).abs() <= bd + 1e-6).all())


def test_restated_gradients_match_the_reference_pytorch_loop():
    """The reference's own march loop (mvpraymarch.py:391-467, 18 steps, 64 primitives, 65 x 65 rays, gout = 1) is fp32 and its
    validity rule differs at the faces (>= / <=, and tminmax in place of the hit interval), so a sample within DELTA_Y = 1e-6 of a
    face may be taken by one side only.  The restatement names those samples itself (its face margin by primitive and by ray,
    no look at the reference): on this scene they touch 3 rays of 4225 (asserted under 1 %) in 3 primitives, which are left out
    of the comparison.  Measured distance of what remains, relative to each tensor's largest entry: template 2.5e-6, primpos
    1.7e-6, primrot 2.9e-6, primscale 2.6e-6 (the fp32 loop's own rounding over ~270 samples per ray).  Bounds: 4 x those."""
    g, z = np.load(os.path.join(GOLDEN, "raymarch.npz")), np.load(os.path.join(GOLDEN, "raymarch_grad.npz"))
    T = lambda k: torch.from_numpy(g[k])[:1]
    tpl = T("march_template").permute(0, 1, 3, 4, 5, 2).contiguous()
    rot, rd = torch.from_numpy(z["primrot"]), torch.from_numpy(z["raydir"])      # (last-bit variants of raymarch.npz's: see the generator)
    assert float((rot - T("march_primrot")).abs().max()) < 1e-6 and float((rd - T("march_raydir")).abs().max()) < 1e-6
    got, img, info = G.grads(T("march_raypos"), rd, T("march_tminmax"), float(g["march_stepsize"]), T("march_primpos"), rot,
                             T("march_primscale"), tpl, torch.ones(1, 65, 65, 4), float(g["march_fadescale"]), float(g["march_fadeexp"]))
    assert float((img - T("march_rgba").double()).abs().max()) < 1e-5
    near_prim, near_ray = info["face_prim"][0] < rr.DELTA_Y, info["face_ray"][0] < rr.DELTA_Y
    print(f"within DELTA_Y of a face: {int(near_ray.sum())} of {near_ray.numel()} rays, primitives {near_prim.nonzero().flatten().tolist()}")
    assert float(near_ray.float().mean()) < 0.01 and int(near_prim.sum()) <= 3
    keep = ~near_prim
    ref = (torch.from_numpy(z["grad_template"]).permute(0, 1, 3, 4, 5, 2), torch.from_numpy(z["grad_primpos"]),
           torch.from_numpy(z["grad_primrot"]), torch.from_numpy(z["grad_primscale"]))
    for name, a, r, bound in zip(TG.NAMES, got, ref, (4 * 2.5e-6, 4 * 1.7e-6, 4 * 2.9e-6, 4 * 2.6e-6)):
        top = float(r.abs().max())
        err = float((a[0][keep] - r[0][keep].double()).abs().max())
        print(f"restatement vs reference loop, {name}: {err / top:.2e} of the largest entry {top:.3e} (bound {bound:.1e})")
        assert top > 0 and err <= bound * top, (name, err / top)


# ------------------------------------------------------------------------------------------------ (b) scene margins
@pytest.mark.parametrize("name", list(TG.SCENES))
def test_gpu_scenes_keep_their_decision_margins(name):
    """Every decision of every GPU scene is at least 1e-5 from its threshold (10 x DELTA_Y of the replay, and far above the fp32
    error of acc.w at these sample counts), so the fp32 kernel takes the samples the float64 restatement takes.  And each scene
    reaches what it is there for."""
    s = TG.build_scene(name)
    with torch.no_grad():
        img, i = G.march(s["rp"], s["rd"], s["tm"], s["dt"], s["pos"].double(), s["rot"].double(), s["scale"].double(), s["tpl"].double(),
                         s["fs"], s["fe"])
    print(f"{name}: margins {i['margin']}; {i['taken']} samples, at most {i['samples']} per ray, {i['hit']} rays with samples, "
          f"{i['saturated']} saturated, {i['steps']} steps")
    assert min(i["margin"].values()) >= TG.MARGIN, i["margin"]
    assert i["hit"] > 0 and i["taken"] > 200
    kw = TG.SCENES[name][0]
    if name.startswith("rotated_sat"):
        assert i["saturated"] > 0.2 * i["hit"]
    if name == "unsaturated":
        assert i["saturated"] == 0 and float(img[..., 3].max()) < 0.99
    if name == "ragged_batch2":
        hit = torch.zeros(2, 16, 32, dtype=torch.bool)
        hit[:, :13, :27] = img[..., 3] > 0
        full = torch.zeros(16, 32, dtype=torch.bool)
        full[:8, :24] = True                                            # the tiles that lie wholly inside the 13 x 27 image
        tiles = lambda m: m.reshape(-1, 2, 8, 4, 8).permute(0, 1, 3, 2, 4).reshape(-1, 8, 64)
        some, every = tiles(hit).any(-1), tiles(hit).all(-1)
        assert kw["H"] % 8 and kw["W"] % 8 and bool((some & ~every & tiles(full[None]).all(-1)).any())  # rays without hits inside a tile with hits
        assert bool((some & ~tiles(full[None]).all(-1)).any())          # ... and hits in a ragged tile, next to shadow lanes
    if name == "noncubic":
        assert tuple(s["tpl"].shape[2:5]) == (3, 4, 5)
    if name == "cache_overflow":
        assert i["saturated"] == 0                                      # chunk_sublists' liveness is exact without saturation
        _, _, st = rr.replay(s["rp"], s["rd"], s["tm"], s["dt"], s["pos"], s["rot"], s["scale"], s["tpl"], s["fs"], s["fe"], with_stats=True)
        assert int(rr.chunk_sublists(st["windows"][0], s["dt"]).max()) > 64
    if name == "hitlist_cap":
        trmin, trmax = rr._slab(s["rp"][0].reshape(-1, 3).double(), s["rd"][0].reshape(-1, 3).double(), s["pos"][0].double(),
                                s["rot"][0].double(), s["scale"][0].double())
        assert int((trmin <= trmax).any(0).sum()) > rr.MAXHIT


# ------------------------------------------------------------------------------------------------ (c) training subsample
def test_training_subsample_is_the_reference_formula():
    from topia_xl_amd import raymarch as rm
    H, W, f, B = 13, 18, 4, 3
    base = rm.base_pixel_coords(H, W)
    assert base.shape == (H, W, 2) and base[5, 7].tolist() == [7.0, 5.0]
    torch.manual_seed(123)
    got = rm.training_pixel_coords(base, B, f)
    torch.manual_seed(123)
    draws = [int(torch.randint(0, f - 1, size=())) for _ in range(2 * B)]     # per item x0 then y0, exclusive upper bound f - 1
    assert got.shape == (B, H // f, W // f, 2) and got.is_contiguous()
    assert len(set(draws)) > 1 and max(draws) <= f - 2
    for b in range(B):
        x0, y0 = draws[2 * b], draws[2 * b + 1]
        assert torch.equal(got[b], base[y0:y0 + f * (H // f):f, x0:x0 + f * (W // f):f])
        assert got[b, 0, 0].tolist() == [float(x0), float(y0)]
    # .eval() coordinates are what they were: the centred strided grid, the same for every batch item, no random draw
    m = rm.RayMarcher(H, W, 1.0, ray_subsample_factor=f).eval()
    state = torch.get_rng_state()
    c = m._pixel_coords(B, f, "cpu")
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(c[0], base[f // 2:f // 2 + f * (H // f):f, f // 2:f // 2 + f * (W // f):f]) and torch.equal(c[0], c[2])
    assert torch.equal(m._pixel_coords(B, 1, "cpu")[1], base)


# ------------------------------------------------------------------------------------------------ (d) stream table, (e) ABI
def test_stream_table_is_closed_with_the_backward_case():
    """tests/test_hip_streams.py may not be edited, so tests/test_hip_raymarch_grad.py registers its case in that table when it is
    imported.  With it the closure of tests/test_streamorder_cpu.py holds for the header of ABI 35."""
    from tests import test_hip_streams as TS
    from tests import test_streamorder_cpu as TC
    for name in TG.STREAM_CASES:
        assert name in TS.CASES
    assert "primx_raymarch_backward" in TS.declared()
    TC.test_every_stream_taking_entry_point_is_declared_by_a_case()
    TC.test_every_declared_name_is_a_stream_taking_prototype()
    TC.test_case_table_is_well_formed()
    assert not [n for n, _ in TS.PARAMS if n in TG.STREAM_CASES]      # it runs in its own module, not twice


def test_abi_35_declares_the_backward():
    from topia_xl_amd import _lib
    assert _lib.ABI_VERSION == 35
    sig = _lib.SIGNATURES["primx_raymarch_backward"]
    assert len(sig) == 23 and sig[3] is _lib._f and sig[-1] is _lib._p
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "primx_hip.h")) as fh:
        text = fh.read()
    assert "#define PRIMX_ABI_VERSION 35" in text and "int primx_raymarch_backward(" in text
