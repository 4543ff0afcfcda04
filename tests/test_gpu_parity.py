"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP path, called through the
Python mirror of the reference API (which goes through the C-ABI of libm360.so), against
  (a) the golden fixtures produced by the reference itself (tests/golden/*.npz), and
  (b) the CPU oracle (oracle/ref_path.py) on seeded inputs.

Stated fp32 tolerances: |d rgb|, |d acc| <= 1e-4; |d dist| <= 1e-4 * max(1, |dist|);
per-op kernels are held much tighter (1e-6 .. 1e-5).
"""
import numpy as np
import pytest
import torch
from conftest import (G19_STAGE_NAMES, assert_cov_within_reference_error, assert_within_reference_error, g19_case,
                      oracle_stages)

from mipnerf360_amd import synthetic

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a HIP device")
    from mipnerf360_amd import _lib
    assert _lib.lib().m360_device_count() >= 1
    return torch.device("cuda:0")


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)


def H(t):
    return t.detach().cpu().numpy()


def close(a, b, atol=1e-6, rtol=1e-5):
    a = H(a) if isinstance(a, torch.Tensor) else a
    b = H(b) if isinstance(b, torch.Tensor) else b
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol)


def close_render(rgb, dist, acc, g_rgb, g_dist, g_acc):
    close(rgb, g_rgb, atol=RGB_TOL, rtol=0)
    close(acc, g_acc, atol=RGB_TOL, rtol=0)
    g_dist = H(g_dist) if isinstance(g_dist, torch.Tensor) else g_dist
    assert np.all(np.abs(H(dist) - g_dist) <= 1e-4 * np.maximum(1.0, np.abs(g_dist)))


def dev_rays(d, dev):
    from mipnerf360_amd.intern.ray import Rays
    return Rays(*[D(d[k], dev) for k in synthetic.RAY_FIELDS])


def build_model(sd_np, dev, n, hp, hn, wb):
    from mipnerf360_amd.model import mipNeRF360
    m = mipNeRF360(randomized=False, num_samples=n, hidden_proposal=hp, hidden_nerf=hn, white_bkgd=wb, device=dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    return m


# =============================================================================== golden fixtures
@pytest.mark.parametrize("kind", ["lego", "garden"])
@pytest.mark.parametrize("n", [8, 64, 128])
def test_g1_g2_sampling_and_lift(golden, dev, kind, n):
    from mipnerf360_amd.intern import parameterization as P, ray as R
    g = golden("g1_g2_sampling")
    o, d, r = (D(g[f"{kind}_{k}"], dev) for k in ("origins", "directions", "radii"))
    near, far = D(g[f"{kind}_near"], dev), D(g[f"{kind}_far"], dev)
    near0, far0 = near.clone(), far.clone()
    t, (means, covs) = R.sample_along_rays(o, d, r, n, near, far, False)
    close(t, g[f"{kind}_{n}_t"], atol=0, rtol=2e-6)
    assert torch.equal(near, near0) and torch.equal(far, far0)  # inputs are never mutated
    tm, tv, rv = (D(g[f"{kind}_{n}_{k}"], dev) for k in ("tmean", "tvar", "rvar"))
    mean, cov = P.gaussian_to_xyz(d, tm, tv, rv)
    close(mean, g[f"{kind}_{n}_xyzmean"], atol=1e-7)
    close(cov, g[f"{kind}_{n}_xyzcov"], atol=1e-9, rtol=1e-5)
    # the reference's own contracted Gaussians at every sample count (near = 0 / N = 128: near-denormal variances)
    close(means, g[f"{kind}_{n}_means"])
    # covariances: the tolerance is the reference's own fp32 error against its fp64 evaluation (2.4e-6 ... 5e-5 of the
    # matrix scale on these inputs), not a guessed rtol
    assert_cov_within_reference_error(H(covs), g[f"{kind}_{n}_covs"], g[f"{kind}_{n}_covs64"], what=f"{kind} N={n}")
    close(means, g[f"{kind}_{n}_means64"], atol=2e-6, rtol=1e-6)


@pytest.mark.parametrize("case", ["big", "tiny", "inside"])
def test_g3_contraction(golden, dev, case):
    from mipnerf360_amd.intern import parameterization as P
    g = golden("g3_contract")
    m, c = P.gaussian_contract(D(g[case + "_mean_in"], dev), D(g[case + "_cov_in"], dev))
    close(m, g[case + "_mean_out"])
    close(c, g[case + "_cov_out"], atol=1e-7, rtol=1e-5)
    close(P.contract(D(g[case + "_mean_in"], dev)), g[case + "_mean_out"])


def test_g4_encodings(golden, dev):
    from mipnerf360_amd.intern.encoding import PositionalEncoding, ViewdirectionEncoding
    g = golden("g4_encoding")
    close(PositionalEncoding()(D(g["mean"], dev), D(g["cov"], dev)), g["ipe"], atol=2e-6)
    for lo, hi in ((0, 4), (1, 3)):
        close(ViewdirectionEncoding(lo, hi)(D(g["viewdirs"], dev)), g[f"vd_{lo}_{hi}"], atol=4e-6)


@pytest.mark.parametrize("kind", ["lego", "garden"])
def test_g5_weights_and_composite(golden, dev, kind):
    from mipnerf360_amd.intern import ray as R
    from mipnerf360_amd.model import prop_net
    g = golden("g5_weights_composite")
    t, dens, rgb, dirs = (D(g[f"{kind}_{k}"], dev) for k in ("t", "density", "rgb", "dirs"))
    pn = prop_net(num_samples=dens.shape[1], hidden_proposal=32, device=dev)
    close(pn.density_to_weight(t, dens, dirs), g[f"{kind}_w"], atol=2e-6)
    for wb in (0, 1):
        c, d, a, w = R.volumetric_rendering(rgb, dens, t, dirs, bool(wb))
        tag = f"{kind}_wb{wb}"
        close(c, g[tag + "_rgb"], atol=2e-6), close(a, g[tag + "_acc"], atol=2e-6)
        close(d, g[tag + "_dist"], atol=2e-6), close(w, g[tag + "_w"], atol=2e-6)


def test_g6_resampling(golden, dev):
    from mipnerf360_amd.intern import ray as R
    g = golden("g6_resample")
    t, w = D(g["t"], dev), D(g["w"], dev)
    n = w.shape[-1]
    w_before = w.clone()
    for ns in (n + 1, 16):
        close(R.sorted_piecewise_constant_pdf(t, w + 0.01, ns, randomized=False), g[f"pdf_samples_{ns}"], atol=4e-6)
    close(R.sorted_piecewise_constant_pdf(t, torch.zeros_like(w), n + 1, randomized=False), g["pdf_zero_samples"], atol=4e-6)
    o, d, r = (D(g["rays_" + k], dev) for k in ("origins", "directions", "radii"))
    for pad in (0.01, 0.0):
        new_t, (means, covs) = R.resample_along_rays(o, d, r, t, w, False, pad)
        close(new_t, g[f"resample_t_pad{pad}"], atol=4e-6)
        if pad == 0.01:
            close(means, g["resample_means"], atol=4e-6)
            assert_cov_within_reference_error(H(covs), g["resample_covs"], g["resample_covs64"], what="resampled covs")
    assert torch.equal(w, w_before)


# =============================================================================== G18: NaN / Inf / degenerate inputs
def same_nans_and_close(got, want, atol=4e-6, rtol=1e-5, what=""):
    """NaN exactly where the reference has NaN, Inf exactly where it has Inf (same sign), close elsewhere."""
    got = H(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), \
        f"{what}: NaN pattern differs at {np.argwhere(np.isnan(got) != np.isnan(want))[:8].tolist()}"
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), f"{what}: Inf pattern differs"
    ok = ~np.isnan(want) & ~inf
    np.testing.assert_allclose(got[ok], want[ok], atol=atol, rtol=rtol, err_msg=what)


def test_g18_viewdir_encoding_degenerate(golden, dev):
    """intern/encoding.py:69-90: acos of |z| = 1 + 2^-23 is NaN in the theta channels only; NaN / Inf / zero components;
    x + 1e-6 == 0 (0/0 and y/0)."""
    from mipnerf360_amd.intern.encoding import ViewdirectionEncoding
    g = golden("g18_degenerate")
    for lo, hi in ((0, 4), (1, 3)):
        same_nans_and_close(ViewdirectionEncoding(lo, hi)(D(g["vd_in"], dev)), g[f"vd_{lo}_{hi}"], what=f"vd_{lo}_{hi}")


def test_g18_sampling_and_lift_degenerate(golden, dev):
    """intern/ray.py:81-116 with far == near, near = far = 0, far < near, directions = 0, radii = 0;
    intern/parameterization.py:46 (the 1e-10 clamp of |d|^2)."""
    from mipnerf360_amd.intern import parameterization as P, ray as R
    g = golden("g18_degenerate")
    r = {k: D(g["sample_rays_" + k], dev) for k in synthetic.RAY_FIELDS}
    t, (m, c) = R.sample_along_rays(r["origins"], r["directions"], r["radii"], 4, r["near"], r["far"], False)
    same_nans_and_close(t, g["sample_t"], atol=0, rtol=2e-6, what="t")
    same_nans_and_close(m, g["sample_means"], what="means")
    same_nans_and_close(c, g["sample_covs"], atol=1e-9, rtol=2e-3, what="covs")
    mean, cov = P.gaussian_to_xyz(D(g["lift_d"], dev), D(g["lift_tm"], dev), D(g["lift_tv"], dev), D(g["lift_rv"], dev))
    same_nans_and_close(mean, g["lift_mean"], atol=1e-7, what="lift mean")
    same_nans_and_close(cov, g["lift_cov"], atol=1e-9, what="lift cov")


def test_g18_resampling_degenerate(golden, dev):
    """intern/ray.py:12-57,118-153 with a NaN weight (the row collapses onto the first bin edge: no NaN comes out), an
    all-NaN row, +Inf, a negative weight (non-monotone cdf), a sum that overflows."""
    from mipnerf360_amd.intern import ray as R
    g = golden("g18_degenerate")
    t, w = D(g["resample_t"], dev), D(g["resample_w"], dev)
    same_nans_and_close(R.sorted_piecewise_constant_pdf(t, w.clone(), 9, randomized=False), g["pdf_samples"], what="pdf 9")
    same_nans_and_close(R.sorted_piecewise_constant_pdf(t, w.clone(), 5, randomized=False), g["pdf_samples_5"], what="pdf 5")
    o, d, r = (D(g["resample_rays_" + k], dev) for k in ("origins", "directions", "radii"))
    new_t, (m, c) = R.resample_along_rays(o, d, r, t, w, False, 0.01)
    same_nans_and_close(new_t, g["resample_new_t"], what="resample t")
    same_nans_and_close(m, g["resample_means"], what="means")
    same_nans_and_close(c, g["resample_covs"], atol=1e-7, rtol=2e-3, what="covs")


def test_g18_weights_and_composite_degenerate(golden, dev):
    """model.py:59-78, intern/ray.py:155-191 with NaN / +Inf / 1e38 / -1e4 densities, a NaN colour, a zero direction:
    NaN weights exactly where the reference has them, the distance never NaN (nan_to_num + clamp, ray.py:187)."""
    from mipnerf360_amd.intern import ray as R
    from mipnerf360_amd.model import prop_net
    g = golden("g18_degenerate")
    t, dens, rgb, dirs = (D(g["render_" + k], dev) for k in ("t", "density", "rgb", "dirs"))
    pn = prop_net(num_samples=dens.shape[1], hidden_proposal=32, device=dev)
    same_nans_and_close(pn.density_to_weight(t, dens, dirs), g["render_w_prop"], what="prop weights")
    for wb in (0, 1):
        c, d, a, w = R.volumetric_rendering(rgb, dens, t, dirs, bool(wb))
        tag = f"render_wb{wb}"
        same_nans_and_close(c, g[tag + "_rgb"], what="rgb"), same_nans_and_close(a, g[tag + "_acc"], what="acc")
        same_nans_and_close(d, g[tag + "_dist"], what="dist"), same_nans_and_close(w, g[tag + "_w"], what="w")


@pytest.mark.parametrize("mlp_dtype", ["bf16x3", "bf16"])
@pytest.mark.parametrize("tag", ["local", "nan_origin", "nan_direction"])
def test_g18_stage_forwards_degenerate_reduced_precision(golden, dev, tag, mlp_dtype):
    """The same batches in the bf16 modes: NaN EXACTLY where the reference has it.  The bf16 matrix pipe answers a NaN operand with
    0xFFC00000, which its integer-max ReLU reads as negative (tools/diag/nan_bits_bf16.py: no NaN survives a ReLU layer there; found in
    round 4 - until then a |z| > 1 view direction rendered finite values in these modes), so the encoder flags the samples that carry a
    NaN feature and the finishers poison their head outputs, where nn.ReLU (model.py:43-53,131-148) would have delivered the NaN.
    Finite values: the modes' own tolerances against the reference's fp32 outputs."""
    from mipnerf360_amd.model import mipNeRF360
    g = golden("g18_degenerate")
    n, hp, hn = (int(x) for x in g["e2e_cfg"])
    m = mipNeRF360(num_samples=n, hidden_proposal=hp, hidden_nerf=hn, device=dev, mlp_dtype=mlp_dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(g).items()})
    rays = dev_rays({k: g[f"e2e_{tag}_rays_{k}"] for k in synthetic.RAY_FIELDS}, dev)
    tol = dict(atol=2e-2, rtol=2e-2) if mlp_dtype == "bf16" else dict(atol=1e-4, rtol=1e-4)
    with torch.no_grad():
        t_hat, w_hat = m.prop_net.forward(rays)
        out = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
        fused = m(rays)
    same_nans_and_close(t_hat, g[f"e2e_{tag}_t_hat"], atol=0, rtol=2e-6, what="t_hat")
    same_nans_and_close(w_hat, g[f"e2e_{tag}_w_hat"], what="w_hat", **tol)
    for nm, v in zip(("rgb", "dist", "acc", "t_vals", "fine_w", "s_vals"), out):
        same_nans_and_close(v, g[f"e2e_{tag}_{nm}"], what=nm, **tol)
    for nm, v in zip(("rgb", "dist", "acc"), fused):
        same_nans_and_close(v, g[f"e2e_{tag}_{nm}"], what="fused " + nm, **tol)


@pytest.mark.parametrize("tag", ["local", "nan_origin", "nan_direction"])
def test_g18_stage_forwards_degenerate(golden, dev, tag):
    """Both stage forwards and the fused forward on a batch that holds degenerate rays: viewdir |z| > 1 (NaN features ->
    the ray is NaN through both MLPs, its resampled t collapses to t[0]), far == near, directions = 0, radii = 0; a NaN
    origin stays local (origins are added after the contraction), a NaN direction enters the whole-chunk norm and turns
    every ray NaN - exactly as in the reference."""
    g = golden("g18_degenerate")
    n, hp, hn = (int(x) for x in g["e2e_cfg"])
    m = build_model(_sd(g), dev, n, hp, hn, False)
    rays = dev_rays({k: g[f"e2e_{tag}_rays_{k}"] for k in synthetic.RAY_FIELDS}, dev)
    with torch.no_grad():
        t_hat, w_hat = m.prop_net.forward(rays)
        out = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
        fused = m(rays)
    same_nans_and_close(t_hat, g[f"e2e_{tag}_t_hat"], atol=0, rtol=2e-6, what="t_hat")
    same_nans_and_close(w_hat, g[f"e2e_{tag}_w_hat"], atol=5e-6, what="w_hat")
    for nm, v in zip(("rgb", "dist", "acc", "t_vals", "fine_w", "s_vals"), out):
        same_nans_and_close(v, g[f"e2e_{tag}_{nm}"], atol=2e-5, rtol=1e-4, what=nm)
    for nm, v in zip(("rgb", "dist", "acc"), fused):
        same_nans_and_close(v, g[f"e2e_{tag}_{nm}"], atol=2e-5, rtol=1e-4, what="fused " + nm)
    # the tape-keeping forward (training) treats them the same way
    t2, w2 = m.prop_net.forward(rays)
    taped = m.nerf_net.forward(rays, t_vals=t2, coarse_weights=w2)
    for nm, v in zip(("rgb", "dist", "acc", "t_vals", "fine_w", "s_vals"), taped):
        same_nans_and_close(v.detach(), g[f"e2e_{tag}_{nm}"], atol=2e-5, rtol=1e-4, what="taped " + nm)


def _sd(g):
    return {k[3:]: v for k, v in g.items() if k.startswith("sd.")}


@pytest.mark.parametrize("kind", ["lego", "garden"])
def test_g7_stage_outputs(golden, dev, kind):
    g = golden("g7_stages_small")
    B, n, wb = (int(x) for x in g[kind + "_cfg"])
    m = build_model(_sd(g), dev, n, 32, 64, bool(wb))
    rays = dev_rays({k: g[f"{kind}_rays_{k}"] for k in synthetic.RAY_FIELDS}, dev)
    t_hat, w_hat = m.prop_net.forward(rays)
    close(t_hat, g[kind + "_t_hat"], atol=0, rtol=2e-6)
    close(w_hat, g[kind + "_w_hat"], atol=5e-6)
    out = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    for nm, v in zip(("rgb", "dist", "acc", "t_vals", "fine_w", "s_vals"), out):
        close(v, g[f"{kind}_{nm}"], atol=2e-5, rtol=1e-4)
    # stashed attributes of the reference (model.py:192-196)
    assert m.nerf_net.fine_weights is out[4] and m.nerf_net.t_vals is out[3] and m.nerf_net.s_vals is out[5]
    # fused whole forward == staged forward
    rgb, dist, acc = m(rays)
    close_render(rgb, dist, acc, g[kind + "_rgb"], g[kind + "_dist"], g[kind + "_acc"])
    close(rgb, out[0], atol=1e-6), close(acc, out[2], atol=1e-6)


@pytest.mark.parametrize("kind,n", [("lego", 64), ("garden", 128)])
def test_g8_end_to_end_full_width(golden, dev, kind, n):
    g = golden("g8_end_to_end_fullwidth")
    B, n_, wb = (int(x) for x in g[f"{kind}_{n}_cfg"])
    m = build_model(synthetic.make_state_dict(256, 1024, seed=int(g["weights_seed"][0])), dev, n_, 256, 1024, bool(wb))
    rays = dev_rays(synthetic.make_rays(kind, B, seed=int(g["rays_seed"][0])), dev)
    rgb, dist, acc = m(rays)
    assert rgb.shape == (B, 3) and dist.shape == (B,) and acc.shape == (B,)
    close_render(rgb, dist, acc, g[f"{kind}_{n}_rgb"], g[f"{kind}_{n}_dist"], g[f"{kind}_{n}_acc"])


@pytest.mark.parametrize("chunks", [128, 4096])
def test_g9_render_image(golden, dev, chunks):
    g = golden("g9_render_image")
    h, w, n = (int(x) for x in g["cfg"])
    m = build_model(_sd(g), dev, n, 32, 64, False)
    from mipnerf360_amd.intern.ray import Rays
    rays_cpu = Rays(*[torch.from_numpy(g["rays_" + k]) for k in synthetic.RAY_FIELDS])  # host rays, like test.py
    rgb8, dist, acc = m.render_image(rays_cpu, h, w, chunks=chunks)
    assert isinstance(rgb8, np.ndarray) and rgb8.dtype == np.uint8 and rgb8.shape == (h, w, 3)
    assert dist.dtype == np.float32 and dist.shape == (h, w) and acc.dtype == np.float32 and acc.shape == (h, w)
    assert np.abs(rgb8.astype(int) - g[f"c{chunks}_rgb8"].astype(int)).max() <= 1
    assert (rgb8 != g[f"c{chunks}_rgb8"]).mean() < 0.02
    close(acc, g[f"c{chunks}_acc"], atol=RGB_TOL, rtol=0)
    close(dist, g[f"c{chunks}_dist"], atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("chunks", [128, 4096])
def test_g9_render_image_bf16x3(golden, dev, chunks):
    """render_image (model.py:254-274) in bf16x3 mode against the reference's frames (fixture G9), both chunk sizes: the
    chunk partition (per-chunk contraction norms, many chunks per launch) is the fp32 path's; the MLP arithmetic keeps the
    frame inside the same tolerances - the uint8 image within one level, distance / acc within 1e-4."""
    from mipnerf360_amd.intern.ray import Rays
    from mipnerf360_amd.model import mipNeRF360
    g = golden("g9_render_image")
    h, w, n = (int(x) for x in g["cfg"])
    m = mipNeRF360(num_samples=n, hidden_proposal=32, hidden_nerf=64, device=dev, mlp_dtype="bf16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(g).items()})
    rays_cpu = Rays(*[torch.from_numpy(g["rays_" + k]) for k in synthetic.RAY_FIELDS])
    rgb8, dist, acc = m.render_image(rays_cpu, h, w, chunks=chunks)
    assert rgb8.dtype == np.uint8 and rgb8.shape == (h, w, 3)
    assert np.abs(rgb8.astype(int) - g[f"c{chunks}_rgb8"].astype(int)).max() <= 1
    assert (rgb8 != g[f"c{chunks}_rgb8"]).mean() < 0.02
    close(acc, g[f"c{chunks}_acc"], atol=RGB_TOL, rtol=0)
    close(dist, g[f"c{chunks}_dist"], atol=1e-4, rtol=1e-4)


# =============================================================================== finishers: one wave per ray
@pytest.mark.parametrize("B,N,width", [(11, 128, 1024), (5, 64, 256), (9, 33, 512)])
def test_finishers_wave_per_ray_match_one_ray_at_a_time(dev, B, N, width):
    """Round 4: a finisher workgroup takes four rays, one wave each, when the fused last layer covered all their samples.  Which
    wave / workgroup a ray lands on must not matter: the batch call equals every ray finished alone (its own launch: wave 0 of
    workgroup 0) BIT FOR BIT, proposal and NeRF finisher, including the t_vals + 1e-6 / s_vals the NeRF finisher now writes
    (against m360_t_to_s).  (The slot order of the partial sums is pinned by the whole-path bit-identity tests.)"""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator().manual_seed(B * N)
    S = B * N
    slots = 2 * width // 256
    r = synthetic.make_rays("lego", B, seed=B)
    rays = dev_rays(r, dev)
    t = torch.sort(torch.rand(B, N + 1, generator=g) * 4 + 2, dim=1).values.to(dev)
    for heads in (1, 4):
        part = (torch.randn(S, slots, heads, generator=g) * 0.7).to(dev)
        hw = torch.zeros(heads, width, device=dev)
        hb = torch.randn(heads, generator=g).to(dev)
        act = torch.zeros(1, width, device=dev)                      # never read: every row is fused
        if heads == 1:
            w, t_new = ops.prop_finish_fused(act, part.reshape(S, slots), S, hw, hb, -1.0, t, rays.directions, 0.01)
            for b in range(B):
                wb, tb = ops.prop_finish_fused(act, part[b * N:(b + 1) * N].reshape(N, slots).contiguous(), N, hw, hb, -1.0, t[b:b + 1].contiguous(),
                                               rays.directions[b:b + 1].contiguous(), 0.01)
                assert torch.equal(wb[0], w[b]) and torch.equal(tb[0], t_new[b]), b
            assert torch.isfinite(w).all() and bool((t_new[:, 1:] >= t_new[:, :-1]).all())
        else:
            out = ops.nerf_finish_outputs(act, part.reshape(S, slots, 4), S, hw, hb, -1.0, 0.001, t, rays.directions, rays.near, rays.far, True)
            for b in range(B):
                ob = ops.nerf_finish_outputs(act, part[b * N:(b + 1) * N].contiguous(), N, hw, hb, -1.0, 0.001, t[b:b + 1].contiguous(),
                                             rays.directions[b:b + 1].contiguous(), rays.near[b:b + 1].contiguous(), rays.far[b:b + 1].contiguous(), True)
                for a, c in zip(out, ob):
                    assert torch.equal(a[b], c[0]), b
            assert torch.equal(out[4], t + 1e-6) and torch.equal(out[5], ops.t_to_s(t, rays.near, rays.far, 1, 1))
            plain = ops.nerf_finish_fused(act, part.reshape(S, slots, 4), S, hw, hb, -1.0, 0.001, t, rays.directions, True)
            for a, c in zip(plain, out[:4]):
                assert torch.equal(a, c)


# =============================================================================== NaN parameters
@pytest.mark.parametrize("mlp_dtype", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("where", ["nerf_net.model.4.weight", "prop_net.model.2.bias", "nerf_net.model.0.weight"])
def test_negative_nan_parameter_propagates_like_nn_relu(dev, mlp_dtype, where):
    """a checkpoint may hold NaN parameters with the SIGN bit set (x86's 0/0 is 0xFFC00000).  nn.ReLU propagates every NaN
    (model.py:43-53,131-148), so the reference renders NaN; the fp32 ReLU epilogues are an integer max on the bit pattern, which keeps
    only NaNs with a clear sign bit - the packing kernels therefore canonicalise NaN parameters to +NaN, and the fp32 path renders NaN
    exactly where the oracle does.  The bf16 modes cannot carry a NaN parameter through their ReLU layers (the bf16 matrix pipe's NaN
    has the sign bit set): they REFUSE such a checkpoint instead of rendering finite values."""
    from oracle import ref_path as O
    sd = synthetic.make_state_dict(64, 128, seed=77)
    neg_nan = np.frombuffer(np.uint32(0xFFC00000).tobytes(), dtype=np.float32)[0]
    assert np.isnan(neg_nan) and np.signbit(neg_nan)
    sd[where] = sd[where].copy()
    sd[where].reshape(-1)[3] = neg_nan
    m = _g19_model(sd, dev, 16, 64, 128, False, mlp_dtype)
    r = synthetic.make_rays("lego", 40, seed=78)
    if mlp_dtype != "fp32":
        with pytest.raises(RuntimeError, match="parameters hold NaN"):
            with torch.no_grad():
                m(dev_rays(r, dev))
        return
    with torch.no_grad():
        rgb, dist, acc = m(dev_rays(r, dev))
    o_rgb, o_dist, o_acc = O.forward(O.rays_from_numpy(r), O.to_torch_state_dict(sd), O.Hyper(num_samples=16))
    # NeRF-net NaN: every ray renders NaN; proposal-net NaN: w_hat is NaN, the resampled t collapse onto t[0] (intern/ray.py:43-50 on a
    # NaN cdf) and the NeRF stage renders finite values from there - either way exactly where the oracle (= nn.ReLU semantics) has them
    assert bool(torch.isnan(o_rgb).all()) == where.startswith("nerf_net")
    assert torch.equal(torch.isnan(rgb).cpu(), torch.isnan(o_rgb)) and torch.equal(torch.isnan(acc).cpu(), torch.isnan(o_acc))
    assert bool(torch.isfinite(dist).all()) and bool(torch.isfinite(o_dist).all())   # nan_to_num + clamp (intern/ray.py:187)
    if not where.startswith("nerf_net"):
        close_render(rgb, dist, acc, o_rgb, o_dist, o_acc)


# =============================================================================== one-launch prologue
@pytest.mark.parametrize("mlp_dtype", ["fp32", "bf16x3"])
def test_fused_prologue_matches_the_separate_kernels_bit_for_bit(dev, mlp_dtype):
    """Round 4: the rendering forward of a large chunk starts with ONE prologue launch (t, view-direction encoding, the norm's partial
    sums from t RECOMPUTED instead of read back, queue words) and the encoder's workgroups take the norm's final sum themselves.
    Against the separate entry points, which still exist: t_hat == m360_sample_t bit for bit, and the proposal weights / resampled t ==
    m360_prop_forward_from_t fed with the norm that m360_mean_sumsq computes with norm_partial_from_t_kernel + norm_final_kernel (the
    same partition and order: the same bits), NeRF stage likewise."""
    from mipnerf360_amd import ops
    B, N = 2048, 128                      # 262 144 samples: above the one-workgroup norm's 131 072
    sd = synthetic.make_state_dict(64, 128, seed=21)
    m = _g19_model(sd, dev, N, 64, 128, False, mlp_dtype)
    rays = dev_rays(synthetic.make_rays("lego", B, seed=22), dev)
    with torch.no_grad():
        t_hat, w_hat = m.prop_net.forward(rays)
        out = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
        rgb, dist, acc = m(rays)
        assert torch.equal(t_hat, ops.sample_t(rays.near, rays.far, N))
        norm0 = m.sharded_sumsq(rays, t_hat).sqrt().float()
        w2, t_new = m.sharded_prop(rays, t_hat, norm0)
        assert torch.equal(w2, w_hat)
        norm1 = m.sharded_sumsq(rays, t_new).sqrt().float()
        rgb2, dist2, acc2 = m.sharded_nerf(rays, t_new, norm1)
    for a, b in ((rgb2, out[0]), (dist2, out[1]), (acc2, out[2]), (rgb, out[0]), (dist, out[1]), (acc, out[2])):
        assert torch.equal(a, b)
    assert torch.equal(out[3], t_new + 1e-6)


# =============================================================================== x6: first layers of the bf16 modes
def test_x6_feature_rows_and_weight_packing(dev):
    """Row format 3 of the encoder and m360_pack_linear_bf16x6: three bf16 terms per value (exact: hi + mid + lo == the fp32
    value), blocks in the order [lo | mid | hi | mid | hi | hi] / [Wh | Wm | Wl | Wh | Wm | Wh]."""
    from mipnerf360_amd import ops
    r = synthetic.make_rays("lego", 70, seed=41)
    rays = dev_rays(r, dev)
    n = 24
    t = ops.sample_t(rays.near, rays.far, n)
    vd = ops.viewdir_enc(rays.viewdirs, 0, 4)
    f32 = ops.encode_features(t, rays.origins, rays.directions, rays.radii, vd, 64)
    x6 = ops.encode_features(t, rays.origins, rays.directions, rays.radii, vd, 64, row_format=3)
    assert x6.shape == (70 * n, 384) and x6.dtype == torch.bfloat16
    assert torch.equal(x6, ops.split_bf16x6(f32))
    lo, mid, hi = x6[:, :64].float(), x6[:, 64:128].float(), x6[:, 128:192].float()
    assert torch.equal(hi + mid + lo, f32)                     # all 24 bits
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(200, 58, generator=g) * 3).to(dev)
    b = torch.randn(200, generator=g).to(dev)
    w[3, 7] = float("inf")
    wp, bp = ops.pack_linear_bf16x6(w, b, 256, 64)
    assert wp.shape == (256, 384) and torch.equal(bp[:200], b) and float(bp[200:].abs().max()) == 0.0
    wh, wm, wl = wp[:, :64].float(), wp[:, 64:128].float(), wp[:, 128:192].float()
    assert torch.equal(wp[:, 192:256].float(), wh) and torch.equal(wp[:, 256:320].float(), wm) and torch.equal(wp[:, 320:].float(), wh)
    ref = torch.zeros(256, 64, device=dev)
    ref[:200, :58] = w
    fin = torch.isfinite(ref)
    assert torch.equal((wh + wm + wl)[fin], ref[fin]) and wh[3, 7] == float("inf") and wm[3, 7] == 0 and wl[3, 7] == 0


@pytest.mark.parametrize("M,n_out", [(700, 256), (256 * 5 + 33, 1024), (90, 96)])
@pytest.mark.parametrize("split", [False, True])
def test_x6_first_layer_is_an_fp32_product(dev, M, n_out, split):
    """The x6 first layer (m360_linear_bf16 / m360_linear_bf16_split on x6 rows and x6 weights, K = 384: full tiles on the ring
    kernel's plain K loop, ragged rows on the generic kernel) against the fp64 product of the fp32 operands: fp32-level error
    (<= 2e-6 of the row's sum of |x w| + |b|), where bf16 features alone are 1e-3 and two-term features 1e-5 away."""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator().manual_seed(M + n_out)
    x = torch.randn(M, 58, generator=g)
    x = torch.cat([torch.sin(3 * x[:, :42]), x[:, 42:]], 1)          # feature-like magnitudes
    w = torch.randn(n_out, 58, generator=g) * 5
    b = torch.randn(n_out, generator=g)
    xp = torch.zeros(M, 64)
    xp[:, :58] = x
    n_pad = ops.round_up(n_out, 64)
    wp, bp = ops.pack_linear_bf16x6(w.to(dev), b.to(dev), n_pad, 64)
    x6 = ops.split_bf16x6(xp.to(dev))
    if split:
        y = ops.join_bf16x3(ops.linear_bf16_split(x6, wp, bp, _lib.ACT_RELU))
    else:
        y = ops.linear_bf16(x6, wp, bp, _lib.ACT_RELU).float()
    want = torch.relu(x.double() @ w.double().t() + b.double())
    scale = (x.double().abs() @ w.double().abs().t() + b.double().abs())
    out_eps = 2.0 ** -16 if split else 2.0 ** -8                   # the OUTPUT's own rounding: two bf16 terms (16 bits) / one (8)
    err = (y[:, :n_out].cpu().double() - want).abs()
    assert bool((err <= 1.01 * out_eps * want.abs() + 2e-6 * scale).all()), float((err / scale).max())
    if n_pad > n_out:
        assert float(y[:, n_out:n_pad].abs().max()) == 0.0


@pytest.mark.parametrize("M,width,k", [(256 * 3 + 57, 512, 256), (256 * 6, 1024, 1024), (256 * 2 + 1, 256, 384)])
def test_paired_rows_of_the_bf16_layers_are_a_permutation(dev, M, width, k):
    """include/m360.h "paired rows" (M360_ROWS_PAIRED_IN / _OUT): the ring kernel reads and writes the same numbers, 64-byte quarters
    of every 2-row x 64-column block of the full tiles transposed - for m360_linear_bf16, m360_linear_bf16x3, the first-layer calls
    (out only) and the fused-heads calls (in only).  Bit for bit against the plain calls through ops.pair_rows; ragged rows stay plain."""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator().manual_seed(M + width + k)
    x = torch.randn(M, k, generator=g).to(dev)
    w = (torch.randn(width, k, generator=g) * (2.0 / k) ** 0.5).to(dev)
    b = (torch.randn(width, generator=g) * 0.1).to(dev)
    IN, OUT, RELU = _lib.ROWS_PAIRED_IN, _lib.ROWS_PAIRED_OUT, _lib.ACT_RELU
    # hidden layer, bf16
    wp, bp = ops.pack_linear_bf16(w, b, width, k)
    xb = x.bfloat16()
    y = ops.linear_bf16(xb, wp, bp, RELU)
    assert ops.rows_pairable(_lib.PAIRABLE_LINEAR, width, k)
    assert torch.equal(ops.pair_rows(ops.linear_bf16(xb, wp, bp, RELU | OUT)), y)
    assert torch.equal(ops.linear_bf16(ops.pair_rows(xb), wp, bp, RELU | IN), y)
    assert torch.equal(ops.pair_rows(ops.linear_bf16(ops.pair_rows(xb), wp, bp, RELU | IN | OUT)), y)
    assert M % 256 == 0 or torch.equal(ops.linear_bf16(xb, wp, bp, RELU | OUT)[(M // 256) * 256:], y[(M // 256) * 256:])
    # hidden layer, bf16x3 ([hi | lo] rows in and out)
    w3, b3 = ops.pack_linear_bf16x3(w, b, width, k)
    x3 = ops.split_bf16x3(x)
    y3 = ops.linear_bf16x3(x3, w3, b3, RELU)
    assert ops.rows_pairable(_lib.PAIRABLE_X3, width, k)
    assert torch.equal(ops.pair_rows(ops.linear_bf16x3(ops.pair_rows(x3), w3, b3, RELU | IN | OUT)), y3)
    assert torch.equal(ops.linear_bf16x3(ops.pair_rows(x3), w3, b3, RELU | IN), y3)
    # fused-heads last layers (in only): the same partial sums
    if width <= 1024:
        hw = torch.randn(4, width, generator=g).to(dev)
        for x3_mode, xin, wpk, bpk, kind in ((False, xb, wp, bp, _lib.PAIRABLE_HEADS), (True, x3, w3, b3, _lib.PAIRABLE_HEADS_X3)):
            if not ops.rows_pairable(kind, width, k):
                continue
            _, part, fused = ops.linear_heads_bf16(xin, wpk, bpk, hw, store_y=False, x3=x3_mode)
            _, part_p, fused_p = ops.linear_heads_bf16(ops.pair_rows(xin), wpk, bpk, hw, store_y=False, x3=x3_mode, paired_in=True)
            assert fused == fused_p == (M // 256) * 256 and torch.equal(part, part_p)


@pytest.mark.parametrize("M,width", [(256 * 4 + 100, 256), (256 * 3, 1024)])
def test_paired_rows_out_of_the_first_layers(dev, M, width):
    """The first layers of the two reduced-precision modes (m360_linear_bf16x3_bf16out: [hi | lo] features, one bf16 term out;
    m360_linear_bf16_split: x6 features, [hi | lo] rows out) with M360_ROWS_PAIRED_OUT: the plain call's rows, paired."""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator().manual_seed(M + width)
    x = torch.zeros(M, 64)
    x[:, :58] = torch.randn(M, 58, generator=g)
    w = torch.randn(width, 58, generator=g).to(dev)
    b = torch.randn(width, generator=g).to(dev)
    OUT, RELU = _lib.ROWS_PAIRED_OUT, _lib.ACT_RELU
    w3, b3 = ops.pack_linear_bf16x3(w, b, width, 64)
    x2 = ops.split_bf16x3(x.to(dev))
    assert ops.rows_pairable(_lib.PAIRABLE_X3_BF16OUT, width, 64)
    assert torch.equal(ops.pair_rows(ops.linear_bf16x3_bf16out(x2, w3, b3, RELU | OUT)), ops.linear_bf16x3_bf16out(x2, w3, b3, RELU))
    w6, b6 = ops.pack_linear_bf16x6(w, b, width, 64)
    x6 = ops.split_bf16x6(x.to(dev))
    assert ops.rows_pairable(_lib.PAIRABLE_SPLIT, width, 384)
    assert torch.equal(ops.pair_rows(ops.linear_bf16_split(x6, w6, b6, RELU | OUT)), ops.linear_bf16_split(x6, w6, b6, RELU))
    # round 3's plain 64-deep first layer (m360_linear_bf16 on bf16 features): the same kernel form, still reachable through the C-ABI
    w1, b1 = ops.pack_linear_bf16(w, b, width, 64)
    x1 = x.to(dev).bfloat16()
    assert ops.rows_pairable(_lib.PAIRABLE_LINEAR, width, 64)
    assert torch.equal(ops.pair_rows(ops.linear_bf16(x1, w1, b1, RELU | OUT)), ops.linear_bf16(x1, w1, b1, RELU))
    with pytest.raises(RuntimeError, match="first layers"):
        ops.linear_bf16(x1, w1, b1, RELU | _lib.ROWS_PAIRED_IN)


def test_paired_rows_are_refused_where_no_kernel_takes_them(dev):
    """A shape the one-wave ring kernel does not take, an activation other than ReLU on the way out, paired input of a first layer:
    M360_ERR_INVALID_ARGUMENT with the reason, never a silently plain result."""
    from mipnerf360_amd import _lib, ops
    IN, OUT, RELU = _lib.ROWS_PAIRED_IN, _lib.ROWS_PAIRED_OUT, _lib.ACT_RELU
    x = torch.randn(512, 192, device=dev).bfloat16()
    wp, bp = ops.pack_linear_bf16(torch.randn(256, 192, device=dev), None, 256, 192)          # K = 192: the ping-pong kernel's
    assert not ops.rows_pairable(_lib.PAIRABLE_LINEAR, 256, 192)
    with pytest.raises(RuntimeError, match="paired rows"):
        ops.linear_bf16(x, wp, bp, RELU | OUT)
    x = torch.randn(512, 256, device=dev).bfloat16()
    wp, bp = ops.pack_linear_bf16(torch.randn(256, 256, device=dev), None, 256, 256)
    with pytest.raises(RuntimeError, match="ReLU"):
        ops.linear_bf16(x, wp, bp, _lib.ACT_NONE | OUT)
    wq, bq = ops.pack_linear_bf16(torch.randn(96, 256, device=dev), None, 128, 256)           # 128 wide: no full tile
    with pytest.raises(RuntimeError, match="paired rows"):
        ops.linear_bf16(x, wq, bq, RELU | IN)
    x6 = ops.split_bf16x6(torch.randn(512, 64, device=dev))
    w6, b6 = ops.pack_linear_bf16x6(torch.randn(256, 58, device=dev), None, 256, 64)
    with pytest.raises(RuntimeError, match="output only"):
        ops.linear_bf16_split(x6, w6, b6, RELU | IN)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_forward_is_the_same_bits_with_and_without_paired_rows(dev, mode):
    """m360_forward in the reduced-precision modes uses paired rows between the layers of both MLPs (full width: every layer on the
    ring kernel); M360_TUNE_PLAIN_ROWS (ops.set_paired_rows(False)) keeps plain rows: the six outputs must not differ in a bit - 1000 rays x 32 samples, i.e.
    125 full tiles + 0 ragged rows for the NeRF stage, and 999 x 33 with ragged rows in every layer."""
    from mipnerf360_amd import ops
    from mipnerf360_amd.model import mipNeRF360
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(256, 1024, seed=5).items()}
    for B, N in ((1000, 32), (999, 33)):
        model = mipNeRF360(num_samples=N, hidden_proposal=256, hidden_nerf=1024, mlp_dtype=mode, device=dev, randomized=False).eval()
        model.load_state_dict(sd)
        rays = dev_rays(synthetic.make_rays("garden", B, seed=3), dev)
        outs = {}
        for on in (True, False):
            was = ops.set_paired_rows(on)
            try:
                with torch.no_grad():
                    outs[on] = [o.clone() for o in model(rays)]
            finally:
                ops.set_paired_rows(was)
        for a, b in zip(outs[True], outs[False]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("M,width,layers", [(32768, 1024, 6), (65536, 1024, 3), (32768, 1024, 1), (131072, 256, 2), (262144, 256, 5)])
def test_hidden_layer_chain_in_one_launch(dev, M, width, layers):
    """m360_mlp_chain_bf16: `layers` equally shaped ReLU layers (1024 wide: the NeRF MLP's; 256 wide: the proposal MLP's) in ONE launch, a
    row block's next layer waiting for the workgroups of its XCD instead of a kernel boundary - bit for bit what `layers` calls of
    m360_linear_bf16 on paired rows give, repeatedly (the hand-over through the L2 has no second chance to be wrong quietly: three runs,
    fresh inputs each)."""
    from mipnerf360_amd import _lib, ops
    if not ops.mlp_chain_bf16_supported(M, width, layers):
        pytest.skip("needs a 256-CU device whose workgroup b runs on XCD b % 8")
    assert not ops.mlp_chain_bf16_supported(M + 256, width, layers) and not ops.mlp_chain_bf16_supported(M, 512, layers)
    g = torch.Generator().manual_seed(M + layers)
    packs = []
    for _ in range(layers):
        w = (torch.randn(width, width, generator=g) * (2.0 / width) ** 0.5).to(dev)
        b = (torch.randn(width, generator=g) * 0.1).to(dev)
        packs.append(ops.pack_linear_bf16(w, b, width, width))
    flags = _lib.ACT_RELU | _lib.ROWS_PAIRED_IN | _lib.ROWS_PAIRED_OUT
    for rep in range(3):
        x = ops.pair_rows(torch.randn(M, width, generator=g).to(dev).bfloat16())
        want = x
        for wp, bp in packs:
            want = ops.linear_bf16(want, wp, bp, flags)
        a, b2 = x.clone(), torch.full_like(x, float("nan"))
        got = ops.mlp_chain_bf16(a, b2, packs)
        assert torch.equal(got, want), (rep, int((got != want).sum()))


@pytest.mark.parametrize("B,N", [(1024, 128), (300, 128), (1024, 33)])
def test_forward_is_the_same_bits_with_and_without_the_hidden_chain(dev, B, N):
    """M360_TUNE_NO_HIDDEN_CHAIN (ops.set_hidden_chain): the bf16 forward with the six hidden NeRF layers as one launch (default) against six launches - 131072 rows (all
    in the chain), 38400 (32768 in the chain + 5632 layer by layer) and 33792 rows of 33 samples (ragged rows as well): not a bit may differ."""
    from mipnerf360_amd import ops
    from mipnerf360_amd.model import mipNeRF360
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(256, 1024, seed=8).items()}
    model = mipNeRF360(num_samples=N, hidden_proposal=256, hidden_nerf=1024, mlp_dtype="bf16", device=dev, randomized=False).eval()
    model.load_state_dict(sd)
    rays = dev_rays(synthetic.make_rays("garden", B, seed=5), dev)
    outs = {}
    for on in (1, 0):
        was = ops.set_hidden_chain(bool(on))
        try:
            with torch.no_grad():
                outs[on] = [o.clone() for o in model(rays)]
            assert model.chain_error() is False  # no workgroup of the chain gave up waiting (m360_forward_chain_error)
        finally:
            ops.set_hidden_chain(was)
    for a, b in zip(outs[1], outs[0]):
        assert torch.equal(a, b)


def test_temporal_stores_flag(dev):
    """M360_STORES_TEMPORAL (what the row blocks use): the same rows as with non-temporal stores; refused without paired output rows."""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1024, 256, generator=g).to(dev)
    w = (torch.randn(512, 256, generator=g) * 0.1).to(dev)
    b = torch.randn(512, generator=g).to(dev)
    IN, OUT, T, RELU = _lib.ROWS_PAIRED_IN, _lib.ROWS_PAIRED_OUT, _lib.STORES_TEMPORAL, _lib.ACT_RELU
    wp, bp = ops.pack_linear_bf16(w, b, 512, 256)
    xb = x.bfloat16()
    assert torch.equal(ops.linear_bf16(xb, wp, bp, RELU | OUT | T), ops.linear_bf16(xb, wp, bp, RELU | OUT))
    w3, b3 = ops.pack_linear_bf16x3(w, b, 512, 256)
    x3 = ops.split_bf16x3(x)
    assert torch.equal(ops.linear_bf16x3(x3, w3, b3, RELU | OUT | T), ops.linear_bf16x3(x3, w3, b3, RELU | OUT))
    assert torch.equal(ops.linear_bf16x3_bf16out(x3, w3, b3, RELU | OUT | T), ops.linear_bf16x3_bf16out(x3, w3, b3, RELU | OUT))
    w6, b6 = ops.pack_linear_bf16x6(w[:, :58].contiguous(), b, 512, 64)
    x6 = ops.split_bf16x6(torch.nn.functional.pad(x[:, :58], (0, 6)))
    assert torch.equal(ops.linear_bf16_split(x6, w6, b6, RELU | OUT | T), ops.linear_bf16_split(x6, w6, b6, RELU | OUT))
    with pytest.raises(RuntimeError, match="M360_STORES_TEMPORAL"):
        ops.linear_bf16(xb, wp, bp, RELU | T)


@pytest.mark.parametrize("M,n_out,k_in", [(700, 256, 58), (256 * 5 + 33, 1024, 58), (90, 96, 58), (1024, 256, 200)])
def test_bf16_mode_first_layer_two_terms_in_one_out(dev, M, n_out, k_in):
    """m360_linear_bf16x3_bf16out: the first layer of the bf16 mode - [hi | lo] features, [Wh | Wh | Wl] weights, the three products of
    the bf16x3 contract, ONE bf16 term out (full tiles: the ring kernel's X3 loop with the plain epilogue; ragged rows: the generic
    kernel).  Against fp64: the product at 16-bit operand accuracy (<= 4 x 2^-16 of the row's sum of |x w|) plus the output's own bf16
    rounding; and bit for bit the hi half of what m360_linear_bf16x3 writes for the same operands... rounded once instead of split."""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator().manual_seed(M + n_out)
    x = torch.randn(M, k_in, generator=g)
    w = torch.randn(n_out, k_in, generator=g) * 3
    b = torch.randn(n_out, generator=g)
    k_pad, n_pad = ops.round_up(k_in, 64), ops.round_up(n_out, 64)
    xp = torch.zeros(M, k_pad)
    xp[:, :k_in] = x
    wp, bp = ops.pack_linear_bf16x3(w.to(dev), b.to(dev), n_pad, k_pad)
    xs = ops.split_bf16x3(xp.to(dev))
    y = ops.linear_bf16x3_bf16out(xs, wp, bp, _lib.ACT_RELU)
    assert y.shape == (M, n_pad) and y.dtype == torch.bfloat16
    want = torch.relu(x.double() @ w.double().t() + b.double())
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    err = (y[:, :n_out].float().cpu().double() - want).abs()
    assert bool((err <= 1.01 * 2.0 ** -8 * want.abs() + 4 * 2.0 ** -16 * scale).all()), float((err / scale).max())
    full = ops.join_bf16x3(ops.linear_bf16x3(xs, wp, bp, _lib.ACT_RELU))             # the same products, two terms out
    assert bool(((y.float() - full).abs() <= 2.0 ** -8 * full.abs() + 1e-30).all())


# =============================================================================== G19: trained-like weights
G19_KINDS = ["lego", "garden", "mixed"]
# rendered values: the stated fp32 tolerance; stage outputs: c x the reference's own fp32 error against its fp64 run
G19_C = {"fp32": 4.0, "bf16x3": 4.0}
_C2_ORACLE = {}


def _g19_model(sd, dev, n, hp_, hn_, wb, mlp_dtype="fp32"):
    from mipnerf360_amd.model import mipNeRF360
    m = mipNeRF360(randomized=False, num_samples=n, hidden_proposal=hp_, hidden_nerf=hn_, white_bkgd=wb, device=dev, mlp_dtype=mlp_dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


@pytest.mark.parametrize("kind", G19_KINDS)
@pytest.mark.parametrize("scope", ["small", "full"])
def test_g19_structured_weights_fp32(golden, dev, scope, kind):
    """Whole-path parity outside the flat regime (reference: model.py:80-94,163-200,247-252,
    intern/ray.py:136-149,155-191): the HIP path against what the REFERENCE produced on trained-like weights - both stage
    forwards, every output.  Rendered values: the stated fp32 tolerance (1e-4) against the reference's fp32 outputs.  Every
    output: no further from the reference's fp64 run than 4 x the reference's own fp32 run is (the path is ill-conditioned
    here: w_hat of the reference's fp32 run is up to 9e-4 from its fp64 run, resampled t up to 2e-3)."""
    g = golden("g19_structured_weights")
    tag = f"{scope}.{kind}"
    (B, n, wb, hp_, hn_, seed), r, sd = g19_case(g, tag)
    m = _g19_model(sd, dev, n, hp_, hn_, wb)
    rays = dev_rays(r, dev)
    with torch.no_grad():
        t_hat, w_hat = m.prop_net.forward(rays)
        out = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
        rgb, dist, acc = m(rays)
    close(t_hat, g[tag + "_t_hat"], atol=0, rtol=2e-6)
    worst = {}
    for nm, v in zip(G19_STAGE_NAMES, (w_hat,) + tuple(out)):
        worst[nm] = assert_within_reference_error(H(v), g[f"{tag}_{nm}"], g[f"{tag}_{nm}64"], c=G19_C["fp32"], floor=5e-6,
                                                  relative_above_one=nm in ("dist", "t_vals"), what=f"{tag} {nm}")
    print(f"G19 {tag} fp32 (error vs fp64 reference / the fp32 reference's own): " + "  ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in worst.items()))
    close_render(rgb, dist, acc, g[tag + "_rgb"], g[tag + "_dist"], g[tag + "_acc"])
    for a, b in zip((rgb, dist, acc), out[:3]):
        assert torch.equal(a, b)               # fused forward == staged forward, bit for bit


@pytest.mark.parametrize("kind", G19_KINDS)
def test_g19_structured_weights_bf16x3(golden, dev, kind):
    """mlp_dtype="bf16x3" on trained-like weights at full width against the REFERENCE: rendered values inside the stated fp32
    tolerance, every stage output within 4 x the reference's own fp32 error of the reference's fp64 run - the same bound the
    exact-fp32 path is held to (the first layers run at full fp32 accuracy on the matrix pipe)."""
    g = golden("g19_structured_weights")
    tag = "full." + kind
    (B, n, wb, hp_, hn_, seed), r, sd = g19_case(g, tag)
    m = _g19_model(sd, dev, n, hp_, hn_, wb, "bf16x3")
    rays = dev_rays(r, dev)
    with torch.no_grad():
        t_hat, w_hat = m.prop_net.forward(rays)
        out = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    worst = {}
    for nm, v in zip(G19_STAGE_NAMES, (w_hat,) + tuple(out)):
        worst[nm] = assert_within_reference_error(H(v), g[f"{tag}_{nm}"], g[f"{tag}_{nm}64"], c=G19_C["bf16x3"], floor=5e-6,
                                                  relative_above_one=nm in ("dist", "t_vals"), what=f"{tag} {nm}")
    print(f"G19 {tag} bf16x3: " + "  ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in worst.items()))
    close_render(out[0], out[1], out[2], g[tag + "_rgb"], g[tag + "_dist"], g[tag + "_acc"])


@pytest.mark.parametrize("kind", G19_KINDS)
def test_g19_structured_weights_bf16(golden, dev, kind):
    """mlp_dtype="bf16" on trained-like weights at full width against the REFERENCE.  Stated tolerance of the mode in this
    regime: |d rgb| <= 2e-2, |d acc| <= 1e-2, |d distance| <= 2e-2 max(1, |distance|), rms |d rgb| <= 4e-3 (PSNR of the
    build's render against the reference's > 48 dB); the 0.1 dB acceptance is test_psnr_within_tenth_db_of_reference."""
    g = golden("g19_structured_weights")
    tag = "full." + kind
    (B, n, wb, hp_, hn_, seed), r, sd = g19_case(g, tag)
    m = _g19_model(sd, dev, n, hp_, hn_, wb, "bf16")
    with torch.no_grad():
        rgb, dist, acc = m(dev_rays(r, dev))
    d_rgb = np.abs(H(rgb) - g[tag + "_rgb"])
    d_acc = np.abs(H(acc) - g[tag + "_acc"])
    d_dist = np.abs(H(dist) - g[tag + "_dist"]) / np.maximum(1.0, np.abs(g[tag + "_dist"]))
    print(f"G19 {tag} bf16: max |d rgb| {d_rgb.max():.2e} rms {np.sqrt((d_rgb ** 2).mean()):.2e} |d acc| {d_acc.max():.2e} |d dist| {d_dist.max():.2e}")
    assert d_rgb.max() <= 2e-2 and np.sqrt((d_rgb ** 2).mean()) <= 4e-3 and d_acc.max() <= 1e-2 and d_dist.max() <= 2e-2


@pytest.mark.parametrize("mlp_dtype", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("chunks", [128, 4096])
def test_g19_render_image_on_structured_weights(golden, dev, chunks, mlp_dtype):
    """render_image (model.py:254-274) on trained-like weights, both chunk sizes (different contraction norms: the shells sit
    elsewhere), against the reference's frames: uint8 image within one level, acc / distance within 4 x the reference's own
    fp32 error of its fp64 frame."""
    from mipnerf360_amd.intern.ray import Rays
    g = golden("g19_structured_weights")
    h, w, n, hp_, hn_, seed = (int(x) for x in g["frame_cfg"])
    sd = {k[len("frame_sd."):]: v for k, v in g.items() if k.startswith("frame_sd.")}
    m = _g19_model(sd, dev, n, hp_, hn_, True, mlp_dtype)
    rays_cpu = Rays(*[torch.from_numpy(g["frame_rays_" + k]) for k in synthetic.RAY_FIELDS])
    rgb8, dist, acc = m.render_image(rays_cpu, h, w, chunks=chunks)
    want = g[f"frame_c{chunks}_rgb8"]
    if mlp_dtype == "bf16":   # the mode's own tolerance (many chunks per launch at chunks = 128: per-chunk norms, x6 rows, NaN flags)
        assert rgb8.dtype == np.uint8 and np.abs(rgb8.astype(int) - want.astype(int)).max() <= 6 and (np.abs(rgb8.astype(int) - want.astype(int)) > 1).mean() < 0.02
        assert np.abs(acc - g[f"frame_c{chunks}_acc"]).max() <= 1e-2
        assert np.all(np.abs(dist - g[f"frame_c{chunks}_dist"]) <= 2e-2 * np.maximum(1.0, np.abs(g[f"frame_c{chunks}_dist"])))
        return
    assert rgb8.dtype == np.uint8 and np.abs(rgb8.astype(int) - want.astype(int)).max() <= 1 and (rgb8 != want).mean() < 0.02
    assert_within_reference_error(acc, g[f"frame_c{chunks}_acc"], g[f"frame_c{chunks}_acc64"], c=4.0, floor=5e-6, what="acc")
    assert_within_reference_error(dist, g[f"frame_c{chunks}_dist"], g[f"frame_c{chunks}_dist64"], c=4.0, floor=5e-6,
                                  relative_above_one=True, what="distance")


@pytest.mark.parametrize("mlp_dtype", ["fp32", "bf16x3", "bf16"])
def test_c2_headline_batch_on_structured_weights_vs_oracle_as_one_chunk(dev, mlp_dtype):
    """configs[1]'s exact ray batch (seed-1 garden rays, 4096 x 128, full width) as ONE chunk on trained-like weights fitted
    to that chunk (the G19 generator; the reference needs ~10 min for this size, so truth = the oracle in fp64, which
    tests/test_oracle_golden.py pins to the reference's fp64 runs at 2e-6, and the error budget = the oracle's fp32 run
    against it).  fp32 and bf16x3: rendered values within the stated 1e-4, every stage output within 4 x the fp32 oracle's
    own error; bf16: the mode's stated tolerance (see test_g19_structured_weights_bf16)."""
    r = synthetic.make_rays("garden", 4096, seed=1)
    sd = synthetic.make_structured_state_dict(256, 1024, 19, r, 128)
    if not _C2_ORACLE:                           # two CPU passes over 4096 x 128 x full width: once for the three modes
        _C2_ORACLE["o32"] = oracle_stages(r, sd, 128, False, "float32")
        _C2_ORACLE["o64"] = oracle_stages(r, sd, 128, False, "float64")
    o32, o64 = _C2_ORACLE["o32"], _C2_ORACLE["o64"]
    assert o32["rgb"].std(0).mean() >= 0.15
    m = _g19_model(sd, dev, 128, 256, 1024, False, mlp_dtype)
    rays = dev_rays(r, dev)
    with torch.no_grad():
        t_hat, w_hat = m.prop_net.forward(rays)
        out = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    got = dict(zip(G19_STAGE_NAMES, (H(w_hat),) + tuple(H(v) for v in out)))
    if mlp_dtype == "bf16":
        d_rgb = np.abs(got["rgb"] - o64["rgb"])
        assert d_rgb.max() <= 2e-2 and np.sqrt((d_rgb ** 2).mean()) <= 4e-3 and np.abs(got["acc"] - o64["acc"]).max() <= 1e-2
        return
    worst = {}
    for nm in G19_STAGE_NAMES:
        worst[nm] = assert_within_reference_error(got[nm], o32[nm], o64[nm], c=4.0, floor=5e-6, relative_above_one=nm in ("dist", "t_vals"),
                                                  what=f"c2 structured {mlp_dtype} {nm}")
    print(f"c2 structured {mlp_dtype}: " + "  ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in worst.items()))
    close_render(out[0], out[1], out[2], o32["rgb"], o32["dist"], o32["acc"])


# =============================================================================== G21: gradients on structured weights
@pytest.mark.parametrize("kind", ["lego", "mixed"])
def test_g21_training_gradients_on_structured_weights(golden, dev, kind):
    """Row f3 outside the flat regime: the reference's train.py loop body, run unchanged on the mirrors (tape-keeping forwards, the
    hand-written backward of both stages, intern.loss), on the trained-like weights of G19 - every parameter gradient of the proposal
    step (train.py:55-62) and of the NeRF step (:69-80) against the reference's autograd, no further from its fp64 gradients than 4 x
    its own fp32 gradients are (the proposal loss through a density shell is ill-conditioned: the reference's fp32 run is ~1 % of a
    tensor's scale from its fp64 run)."""
    from conftest import assert_grad_within_reference_error, g21_case
    from mipnerf360_amd.intern.loss import Loss_dist, Loss_nerf, Loss_prop
    g = golden("g21_structured_gradients")
    (B, n, wb, hp_, hn_), r, sd, pixels = g21_case(g, kind)
    model = build_model(sd, dev, n, hp_, hn_, wb)
    model.train()
    rays = dev_rays(r, dev)
    t_hat, w_hat = model.prop_net.forward(rays)
    _, _, _, t, w, _ = model.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    loss_prop = Loss_prop(t=t.detach(), w=w.detach(), t_hat=t_hat, w_hat=w_hat)
    model.zero_grad()
    loss_prop.backward()
    lp64, lp32 = float(g[kind + "_loss_prop64"]), float(g[kind + "_loss_prop"])    # the loss itself is ill-conditioned: 0.1-0.2 % fp32 vs fp64
    assert abs(float(loss_prop.detach()) - lp64) <= 4.0 * max(abs(lp32 - lp64), 1e-3 * abs(lp64)), (float(loss_prop.detach()), lp32, lp64)
    worst = 0.0
    for name, p in model.named_parameters():
        if name.startswith("prop_net"):
            e, e_ref = assert_grad_within_reference_error(H(p.grad), g[f"{kind}_propstep.{name}"], g[f"{kind}_propstep64.{name}"], what=f"prop step {name}")
            worst = max(worst, e / max(e_ref, 2e-4))
    model.zero_grad()
    t_hat, w_hat = model.prop_net.forward(rays)
    rgb, _, _, _, fine_w, s_vals = model.nerf_net.forward(rays, t_vals=t_hat.detach(), coarse_weights=w_hat.detach())
    loss_nerf, _ = Loss_nerf(rgb, D(pixels, dev))
    loss_dist = Loss_dist(s_vals, fine_w)
    (loss_nerf + 0.01 * loss_dist).backward()
    close(loss_nerf, g[kind + "_loss_nerf"], rtol=1e-4, atol=0)
    worst_n = 0.0
    for name, p in model.named_parameters():
        if name.startswith("nerf_net"):
            e, e_ref = assert_grad_within_reference_error(H(p.grad), g[f"{kind}_nerfstep.{name}"], g[f"{kind}_nerfstep64.{name}"], what=f"nerf step {name}")
            worst_n = max(worst_n, e / max(e_ref, 2e-4))
    print(f"G21 {kind}: worst gradient error / max(the reference's own fp32 error, 2e-4): proposal step {worst:.2f}, NeRF step {worst_n:.2f}")


# =============================================================================== G20: a trained checkpoint
@pytest.mark.parametrize("mlp_dtype", ["fp32", "bf16x3", "bf16"])
def test_g20_trained_checkpoint_renders_like_the_reference(golden, dev, mlp_dtype):
    """Rows f3 + f4 + the whole path on weights that OPTIMISATION produced: tests/golden/g20_trained_checkpoint.pt was trained on an
    MI355X by the reference's loop body running on the HIP mirrors (tools/train_demo.py, 500 iterations, PSNR 2 -> 29-34 dB), saved
    in the reference's checkpoint layout (train.py:98-103) and rendered by the reference's own class (fixture G20, fp32 + fp64).
    `load_reference_checkpoint` loads the file (architecture inferred from the tensor shapes) and the HIP path renders the 1024
    training rays as ONE chunk: fp32 and bf16x3 within 4 x the reference's own fp32 error on every stage output and inside the stated
    1e-4 on the rendered values; bf16: PSNR within 0.1 dB of the reference's against the training target's noise levels."""
    import json
    import os
    from conftest import GOLDEN_DIR
    from mipnerf360_amd import checkpoint
    g = golden("g20_trained_checkpoint_render")
    meta = json.load(open(os.path.join(GOLDEN_DIR, "g20_training_run.json")))
    B, n, wb, hp_, hn_, seed = (int(x) for x in g["cfg"])
    m = checkpoint.load_reference_checkpoint(os.path.join(GOLDEN_DIR, "g20_trained_checkpoint.pt"), device=dev, num_samples=n,
                                             white_bkgd=bool(wb), mlp_dtype=mlp_dtype)
    assert (m.hidden_proposal, m.hidden_nerf) == (hp_, hn_)
    rays = dev_rays({k: g["rays_" + k] for k in synthetic.RAY_FIELDS}, dev)
    with torch.no_grad():
        t_hat, w_hat = m.prop_net.forward(rays)
        out = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    got = dict(zip(G19_STAGE_NAMES, (H(w_hat),) + tuple(H(v) for v in out)))
    if mlp_dtype == "bf16":
        ref_rgb = g["rgb"].astype(np.float64)
        gen = np.random.Generator(np.random.PCG64(2020))
        worst = 0.0
        for noise in (0.02, 0.1, 0.3):
            target = np.clip(ref_rgb + noise * gen.normal(size=ref_rgb.shape), 0.0, 1.0)
            psnr = lambda a: -10.0 * np.log10(np.mean((np.clip(a, 0, 1) - target) ** 2))  # noqa: E731
            worst = max(worst, abs(psnr(got["rgb"].astype(np.float64)) - psnr(ref_rgb)))
        print(f"G20 bf16: PSNR differs from the reference's by {worst:.5f} dB, max |d rgb| {np.abs(got['rgb'] - g['rgb']).max():.2e}")
        assert worst <= 0.1 and np.abs(got["rgb"] - g["rgb"]).max() <= 2e-2
        return
    worst = {}
    for nm in G19_STAGE_NAMES:
        worst[nm] = assert_within_reference_error(got[nm], g[nm], g[nm + "64"], c=4.0, floor=5e-6, relative_above_one=nm in ("dist", "t_vals"),
                                                  what=f"G20 {mlp_dtype} {nm}")
    print(f"G20 {mlp_dtype}: " + "  ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in worst.items()))
    close_render(out[0], out[1], out[2], g["rgb"], g["dist"], g["acc"])


# =============================================================================== oracle, seeded inputs
def test_linear_mfma_against_fp64(dev):
    """The MFMA GEMM for ragged M / N / K, all activations, vs an fp64 CPU product."""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator().manual_seed(0)
    for M, n_out, k_in, act in [(1, 32, 58, 1), (255, 64, 64, 0), (256, 256, 256, 1), (257, 96, 160, 2),
                                (1000, 1024, 1024, 1), (777, 288, 320, 2), (513, 1, 64, 0)]:
        x = torch.randn(M, k_in, generator=g)
        w = torch.randn(n_out, k_in, generator=g) / k_in ** 0.5
        b = torch.randn(n_out, generator=g)
        k_pad, n_pad = ops.round_up(k_in), ops.round_up(n_out)
        xp = torch.zeros(M, k_pad)
        xp[:, :k_in] = x
        wp, bp = ops.pack_linear(w.to(dev), b.to(dev), n_pad, k_pad)
        assert wp.shape == (n_pad, k_pad) and float(wp[n_out:].abs().sum()) == 0 and float(wp[:, k_in:].abs().sum()) == 0
        y = ops.linear(xp.to(dev), wp, bp, act)
        ref = x.double() @ w.double().T + b.double()
        ref = {0: ref, 1: ref.clamp_min(0), 2: torch.sigmoid(ref)}[act]
        close(y[:, :n_out], ref.float(), atol=2e-5, rtol=2e-5)
        pad_expect = {0: 0.0, 1: 0.0, 2: 0.5}[act]
        if n_pad > n_out:
            assert torch.all(y[:, n_out:] == pad_expect)


@pytest.mark.parametrize("M,n,k,act", [(256 * 37 + 5, 1024, 64, 1), (256 * 530, 256, 64, 0), (256 * 9, 256, 256, 1),
                                        (256 * 64, 1024, 1024, 1), (256, 768, 32, 1), (256 * 3, 512, 96, 0),
                                        (256 * 21 + 255, 768, 64, 1), (256 * 300 + 1, 256, 32, 0),
                                        (256 * 11 + 3, 256, 256, 2), (256 * 40, 1024, 1024, 2),   # sigmoid layers
                                        (128 * 601, 1024, 96, 1), (128 * 3, 256, 64, 0), (128 * 515 + 77, 512, 160, 1),
                                        (128 * 257, 256, 1024, 1), (128, 4096, 64, 1), (128 * 19, 4352, 64, 1),
                                        (128 * 256 * 5 + 128 * 3, 256, 64, 1), (128 * 256 * 9, 512, 96, 0)])   # >= 4 tiles per workgroup: the ticket pool is live
def test_linear_kernel_variants_bit_identical(dev, M, n, k, act):
    """The three fp32 kernels behind m360_linear must agree bit for bit, every element.  The library picks the kernel per
    call from the shape alone (no global switch): full tiles of a 256-multiple width go to the half-tile kernel (bias +
    none / ReLU, contraction >= 64, width <= 4096: 128-row tiles, two accumulator sets, the epilogue of a tile inside the
    next tile's K loop) or to the 256 x 256 persistent kernel (sigmoid, contraction 32, wider layers), ragged rows to the
    workgroup-per-tile kernel.  Blocks of fewer than 128 rows always take the last one, so the same rows are recomputed in
    127-row blocks (and in 255-row blocks: one half tile + 127 ragged rows) and compared."""
    from mipnerf360_amd import ops
    g = torch.Generator(device=dev).manual_seed(M + n + k)
    x = torch.rand(M, k, device=dev, generator=g) * 2 - 1
    w = (torch.rand(n, k, device=dev, generator=g) * 2 - 1) * (6.0 / k) ** 0.5
    b = torch.rand(n, device=dev, generator=g) - 0.5
    wp, bp = ops.pack_linear(w, b)
    xp = torch.zeros(M, wp.shape[1], device=dev)
    xp[:, :k] = x
    y_full = ops.linear(xp, wp, bp, act)
    for _ in range(3):  # repeated launches: a race would not reproduce identically
        assert torch.equal(ops.linear(xp, wp, bp, act), y_full)
    # the XCD-balanced launch (last tiles handed out by ticket: which workgroup computes a tile varies from run to run)
    for _ in range(3):
        assert torch.equal(ops.linear(xp, wp, bp, act, balanced=True), y_full)
    # row blocks spread over the batch (first / middle / last tiles of the persistent walk)
    starts = sorted({0, 128, 256, (M // 512) * 256, max(((M // 256) - 1) * 256, 0), max(((M // 128) - 1) * 128, 0), max(M - 255, 0), max(M - 127, 0)})
    for a in starts:
        for blk in (127, 255):
            rows = min(blk, M - a)
            if rows <= 0:
                continue
            y_blk = ops.linear(xp[a:a + rows], wp, bp, act)
            assert torch.equal(y_blk, y_full[a:a + rows]), f"rows {a}..{a + rows} differ between the kernels"


@pytest.mark.parametrize("M,n,k", [(1024, 256, 64), (1024, 256, 256), (700, 256, 64), (90, 96, 64), (1024, 512, 32)])
def test_linear_relu_lets_nan_rows_through(dev, M, n, k):
    """torch.relu(NaN) is NaN (model.py:43-53,131-148 are nn.ReLU): a sample whose features hold a NaN must come out of
    every ReLU / sigmoid layer as NaN in EVERY unit, in every kernel behind m360_linear (half-tile, 256 x 256 persistent,
    ragged), and must not disturb any other row.  The ReLU is a signed-integer max (include/m360.h): it keeps NaNs with a
    clear sign bit - what the path's encoder writes for every NaN feature (next test) - and the matrix pipe hands a NaN
    operand on with its sign and payload, so such a row stays +NaN through a whole stack of layers."""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator(device=dev).manual_seed(M + n + k)
    x = torch.rand(M, k, device=dev, generator=g) * 2 - 1
    w = (torch.rand(n, k, device=dev, generator=g) * 2 - 1) * (6.0 / k) ** 0.5
    b = torch.rand(n, device=dev, generator=g) - 0.5
    wp, bp = ops.pack_linear(w, b)
    bad = x.clone()
    rows = [5, M // 2 + 3, M - 1]
    bad[rows[0], 3] = float("nan")                        # 0x7FC00000
    bad.view(torch.int32)[rows[1], 7] = 0x7FC12345         # a payload
    bad[rows[2], k - 1] = float("nan")
    for act in (_lib.ACT_RELU, _lib.ACT_SIGMOID, _lib.ACT_NONE):
        clean = ops.linear(x, wp, bp, act)
        y = ops.linear(bad, wp, bp, act)
        assert torch.isnan(y[rows]).all(), f"act {act}: a NaN input row came out with finite units"
        assert (y[rows].view(torch.int32) > 0).all()      # and still with a clear sign bit: the next layer's ReLU keeps it too
        keep = torch.ones(M, dtype=torch.bool, device=dev)
        keep[rows] = False
        assert torch.equal(y[keep], clean[keep])
    # the sign-bit convention, pinned: sigmoid / none keep a negative NaN, the integer-max ReLU reads it as negative
    neg = x.clone()
    neg.view(torch.int32)[5, 3] = -4194304                # 0xFFC00000
    assert torch.isnan(ops.linear(neg, wp, bp, _lib.ACT_NONE)[5]).all()
    assert not torch.isnan(ops.linear(neg, wp, bp, _lib.ACT_RELU)[5]).any()


def test_encoder_writes_every_nan_feature_with_a_clear_sign_bit(dev):
    """The convention the ReLU relies on: whatever the sign of the NaN in the rays (x86 arithmetic produces 0xFFC00000),
    m360_encode_features writes 0x7FC00000 - checked on the features of the fused path's encoder, fp32 and bf16."""
    from mipnerf360_amd import _lib, ops
    r = synthetic.make_rays("garden", 70, seed=5)
    rays = dev_rays(r, dev)
    neg_nan = torch.tensor([-4194304], dtype=torch.int32, device=dev).view(torch.float32)
    rays.origins[3, 1] = neg_nan[0]          # NaN mean (added after the contraction): IPE sin / cos NaN
    rays.radii[9, 0] = neg_nan[0]            # NaN covariance only: the damping factor is NaN
    rays.viewdirs[20] = torch.tensor([0.0, 0.0, -(1.0 + 2.0 ** -23)], device=dev)
    rays.viewdirs[21, 0] = neg_nan[0]
    n = 24
    t = ops.sample_t(rays.near, rays.far, n)
    vd = ops.viewdir_enc(rays.viewdirs, 0, 4)
    feats = [ops.encode_features(t, rays.origins, rays.directions, rays.radii, vd, 64)]
    fb = torch.empty(70 * n, 64, device=dev, dtype=torch.bfloat16)
    ws = torch.empty(_lib.lib().m360_contract_workspace_bytes(), dtype=torch.uint8, device=dev)
    ops.call("m360_encode_features_bf16", t, rays.origins, rays.directions, rays.radii, vd, 16, 70, n, fb, 64, ws, ws.numel(),
             ops.STREAM)
    feats.append(fb)
    for feat in feats:
        f32 = feat.float().view(70, n, 64)
        nan = torch.isnan(f32)
        assert nan[3, :, :42].all() and nan[9, :, :42].all() and nan[20, :, 42:50].all() and nan[21, :, 42:58].any()
        assert not nan[[0, 1, 2, 4, 5]].any()
        bits = f32.contiguous().view(torch.int32)
        assert (bits[nan] > 0).all(), "a NaN feature left the encoder with its sign bit set"


def test_linear_rejects_bad_arguments(dev):
    from mipnerf360_amd import ops
    x = torch.zeros(4, 48, device=dev)
    w = torch.zeros(32, 64, device=dev)
    with pytest.raises(RuntimeError):
        ops.linear(x, w, torch.zeros(32, device=dev))          # K mismatch
    with pytest.raises(RuntimeError):
        ops.linear(torch.zeros(4, 64), w, torch.zeros(32, device=dev))  # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        ops.linear(torch.zeros(4, 64, device=dev).double(), w, torch.zeros(32, device=dev))


@pytest.mark.parametrize("kind,B,n", [("garden", 37, 128), ("lego", 300, 64), ("garden", 5, 200), ("lego", 3, 1)])
def test_sample_encode_vs_oracle(dev, kind, B, n):
    from mipnerf360_amd import ops
    from oracle import ref_path as O
    r = synthetic.make_rays(kind, B, seed=3)
    ro = O.rays_from_numpy(r)
    t_o = O.sample_t(ro.near, ro.far, n).expand(B, -1).contiguous()
    m_o, c_o = O.para_rays(t_o, ro.origins, ro.directions, ro.radii)
    x_o = O.encode_inputs(m_o, c_o, ro.viewdirs)
    rd = dev_rays(r, dev)
    t = ops.sample_t(rd.near, rd.far, n)
    close(t, t_o, atol=0, rtol=2e-6)
    m, c = ops.para_rays(t, rd.origins, rd.directions, rd.radii)
    close(m, m_o, atol=2e-6)
    # covariances against the oracle's formulas evaluated in fp64 on the same fp32 rays: no further than 3 x the fp32
    # oracle's own distance from them
    r64 = O.Rays(*[f.double() for f in ro])
    _, c_64 = O.para_rays(O.sample_t(r64.near, r64.far, n).expand(B, -1).contiguous(), r64.origins, r64.directions, r64.radii)
    assert c_64.dtype == torch.float64
    assert_cov_within_reference_error(H(c), c_o.numpy(), c_64.numpy(), what=f"{kind} B={B} N={n}")
    vd = ops.viewdir_enc(rd.viewdirs, 0, 4)
    close(vd, O.viewdir_enc(ro.viewdirs), atol=4e-6)
    feat = ops.encode_features(t, rd.origins, rd.directions, rd.radii, vd)
    assert feat.shape == (B * n, 64)
    close(feat[:, :58], x_o.reshape(B * n, 58), atol=4e-6)
    assert float(feat[:, 58:].abs().sum()) == 0.0
    # jittered sampling with shared uniforms
    u = torch.rand(B, n + 1, generator=torch.Generator().manual_seed(1))
    close(ops.sample_t(rd.near, rd.far, n, u.to(dev)), O.jitter_t(t_o, u), atol=0, rtol=4e-6)
    # t <-> s helpers
    close(ops.t_to_s(t, rd.near, rd.far, 1, 1), O.t_to_s(t_o, ro.near, ro.far), atol=2e-6, rtol=1e-5)
    close(ops.g(rd.far), O.disparity_eps(ro.far), atol=0, rtol=1e-6)
    s = torch.linspace(0, 1, n + 1)
    close(ops.s_to_t(s.to(dev), rd.near, rd.far), t_o, atol=0, rtol=2e-6)


@pytest.mark.parametrize("B,n", [(9, 128), (130, 64), (4, 257), (6, 1), (5, 2)])
def test_ray_scans_vs_oracle(dev, B, n):
    from mipnerf360_amd import ops
    from oracle import ref_path as O
    g = torch.Generator().manual_seed(B * 1000 + n)
    torch.manual_seed(B * 1000 + n)
    t = torch.sort(torch.rand(B, n + 1, generator=g) * 4 + 2, dim=-1).values
    dens = torch.distributions.Gamma(0.6, 0.25).sample((B, n)).float()
    dens[0] = 0
    rgb = torch.rand(B, n, 3, generator=g)
    dirs = torch.randn(B, 3, generator=g)
    w_o = O.density_to_weight(t, dens, dirs)
    close(ops.density_to_weight(D(t, dev), D(dens, dev), D(dirs, dev)), w_o, atol=2e-6)
    for wb in (False, True):
        out_o = O.volumetric_rendering(rgb, dens[..., None], t, dirs, wb)
        out = ops.volumetric_rendering(D(rgb, dev), D(dens, dev)[..., None], D(t, dev), D(dirs, dev), wb)
        for a, b in zip(out, out_o):
            close(a, b, atol=4e-6, rtol=1e-5)
    w = torch.rand(B, n, generator=g)
    w[0] = 0
    for pad in (0.01, 0.0):
        close(ops.resample_t(D(t, dev), D(w, dev), pad), O.resample_t(t, w, pad), atol=8e-6)
    u = torch.rand(B, n + 1, generator=g)
    close(ops.resample_t(D(t, dev), D(w, dev), 0.01, D(u, dev)), O.resample_t(t, w, 0.01, u), atol=8e-6)
    for ns in (1, 7, n + 1, 300):
        close(ops.sorted_pdf(D(t, dev), D(w, dev) + 0.01, ns), O.sorted_piecewise_constant_pdf(t, w + 0.01, ns), atol=8e-6)
    out = ops.resample_t(D(t, dev), D(w, dev), 0.01)
    assert torch.all(out[:, 1:] >= out[:, :-1])  # sortedness of the resampled t
    assert torch.all(out >= D(t, dev)[:, :1]) and torch.all(out <= D(t, dev)[:, -1:])


def test_to8b_matches_numpy(dev):
    from mipnerf360_amd import ops
    from oracle import ref_path as O
    x = torch.cat([torch.linspace(-0.5, 1.5, 4001), torch.tensor([float("nan"), float("inf"), -float("inf"), 1.0, 0.0,
                                                                  254.5 / 255, 0.999999])])
    assert np.array_equal(H(ops.to8b(x.to(dev))), O.to8b(x.numpy()))


@pytest.mark.parametrize("kind,B,n,hp,hn,wb", [("garden", 96, 128, 256, 1024, False), ("lego", 130, 64, 64, 96, True),
                                               ("garden", 1, 32, 32, 32, False), ("lego", 1024, 128, 256, 1024, True),
                                               ("garden", 40, 256, 64, 128, False),   # BASELINE configs[4]: 256 samples
                                               ("lego", 9, 1, 32, 32, True), ("garden", 5, 3, 32, 64, False),
                                               ("lego", 3, 1000, 32, 32, False)])     # one sample; odd; very long rays
def test_forward_vs_oracle(dev, kind, B, n, hp, hn, wb):
    from oracle import ref_path as O
    sd = synthetic.make_state_dict(hp, hn, seed=5)
    r = synthetic.make_rays(kind, B, seed=8)
    m = build_model(sd, dev, n, hp, hn, wb)
    with torch.no_grad():
        rgb, dist, acc = m(dev_rays(r, dev))
    o = O.forward(O.rays_from_numpy(r), O.to_torch_state_dict(sd), O.Hyper(num_samples=n, white_bkgd=wb))
    close_render(rgb, dist, acc, *o)


def test_randomized_mode_is_statistically_sane(dev):
    """randomized=True cannot share torch's RNG stream with the reference: check the
    jittered pipeline stays close to the deterministic render and differs between calls."""
    from mipnerf360_amd.model import mipNeRF360
    sd = synthetic.make_state_dict(64, 128, seed=2)
    r = dev_rays(synthetic.make_rays("lego", 256, seed=4), dev)
    det = build_model(sd, dev, 64, 64, 128, True)
    rnd = mipNeRF360(randomized=True, num_samples=64, hidden_proposal=64, hidden_nerf=128, white_bkgd=True, device=dev)
    rnd.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    rnd.eval()  # reference quirk: sub-nets keep randomized=True after eval() (model.py:281-283)
    with torch.no_grad():
        a, b, c = det(r)[0], rnd(r)[0], rnd(r)[0]
    assert not torch.equal(b, c)
    assert float((a - b).abs().mean()) < 0.05
    assert torch.isfinite(b).all()


# (randomized=True against the oracle on the uniforms the kernels drew themselves: tests/test_gpu_random.py)


# =============================================================================== BASELINE.json full size
def test_c2_full_size_properties(dev):
    """configs[1]: 4096 rays x 128 samples, full-width fp32 MLPs — properties that do not need the
    CPU oracle at this size: determinism, range, ray-permutation equivariance (the only coupling
    between rays is the permutation-invariant global norm), agreement of a sub-batch rendered
    with the SAME global norm is covered by the equivariance check."""
    sd = synthetic.make_state_dict(256, 1024, seed=0)
    r = synthetic.make_rays("garden", 4096, seed=1)
    m = build_model(sd, dev, 128, 256, 1024, False)
    rays = dev_rays(r, dev)
    with torch.no_grad():  # the fused rendering forward (m360_forward), the one bench.py times
        rgb, dist, acc = m(rays)
        rgb2, dist2, acc2 = m(rays)
    assert not rgb.requires_grad
    assert torch.equal(rgb, rgb2) and torch.equal(dist, dist2) and torch.equal(acc, acc2)
    assert torch.isfinite(rgb).all() and torch.isfinite(dist).all() and torch.isfinite(acc).all()
    assert float(acc.min()) >= 0 and float(acc.max()) <= 1 + 1e-5
    assert float(rgb.min()) >= -0.001 - 1e-6 and float(rgb.max()) <= 1.001 + 1e-6
    tv = m.nerf_net.t_vals
    assert torch.all(tv[:, 1:] >= tv[:, :-1])
    assert torch.all(dist >= tv[:, 0] - 2e-6) and torch.all(dist <= tv[:, -1])
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(0)).to(dev)
    from mipnerf360_amd.intern.ray import Rays
    rp = Rays(*[f[perm].contiguous() for f in rays])
    with torch.no_grad():
        rgb_p, dist_p, acc_p = m(rp)
    close(rgb_p, rgb[perm], atol=2e-5), close(acc_p, acc[perm], atol=2e-5), close(dist_p, dist[perm], atol=2e-5)


def test_c2_headline_batch_vs_oracle_as_one_chunk(dev):
    """configs[1] at its OWN chunk size: bench.py's exact batch (seed-0 weights, seed-1 rays, 4096 x 128, full width)
    through the fused rendering forward (m360_forward under no_grad) against the CPU oracle on all 4096 rays as ONE
    chunk - the contraction norm of intern/parameterization.py:23-29 (called at :75) spans the whole chunk, so a
    sub-batch is a different computation (model.py:247-252).  Stated fp32 tolerance: |d rgb|, |d acc| <= 1e-4,
    |d distance| <= 1e-4 * max(1, |distance|).  Also: the tape-keeping forward (grad enabled) gives the same bits at
    this size, and so do the two stage entry points called one after the other."""
    from oracle import ref_path as O
    sd = synthetic.make_state_dict(256, 1024, seed=0)
    r = synthetic.make_rays("garden", 4096, seed=1)
    m = build_model(sd, dev, 128, 256, 1024, False)
    rays = dev_rays(r, dev)
    with torch.no_grad():
        rgb, dist, acc = m(rays)
        tv, fw, sv = m.nerf_net.t_vals.clone(), m.nerf_net.fine_weights.clone(), m.nerf_net.s_vals.clone()
        t_hat, w_hat = m.prop_net.forward(rays)
        staged = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    assert not rgb.requires_grad
    with torch.no_grad():
        o_sd = O.to_torch_state_dict(sd)
        hp = O.Hyper(num_samples=128)
        o_rays = O.rays_from_numpy(r)
        o_t, o_w = O.prop_forward(o_rays, o_sd, hp)
        o_rgb, o_dist, o_acc, o_tv, o_fw, o_sv = O.nerf_forward(o_rays, o_t, o_w, o_sd, hp)
    close(rgb, o_rgb, atol=1e-4, rtol=0), close(acc, o_acc, atol=1e-4, rtol=0)
    assert float(((dist.cpu() - o_dist).abs() / o_dist.abs().clamp(min=1.0)).max()) <= 1e-4
    close(t_hat, o_t, atol=2e-6, rtol=1e-5), close(w_hat, o_w, atol=2e-5, rtol=1e-4)
    close(tv, o_tv, atol=1e-5, rtol=1e-4), close(fw, o_fw, atol=2e-5, rtol=1e-4), close(sv, o_sv, atol=1e-5, rtol=1e-4)
    for k, ref in enumerate((rgb, dist, acc)):
        assert torch.equal(staged[k], ref)
    del staged, o_rgb, o_tv, o_fw, o_sv
    t2, w2 = m.prop_net.forward(rays)                               # grad enabled: m360_prop_forward_train
    taped = m.nerf_net.forward(rays, t_vals=t2, coarse_weights=w2)  # m360_nerf_forward_train (17 GB tape)
    assert taped[0].requires_grad
    assert torch.equal(t2, t_hat) and torch.equal(w2.detach(), w_hat)
    for k, ref in enumerate((rgb, dist, acc, tv, fw, sv)):
        assert torch.equal(taped[k].detach(), ref), f"tape-keeping forward differs from the fused one in output {k}"


@pytest.mark.parametrize("name,ndc", [("pinhole", False), ("llff", True)])
def test_g10_ray_generation(golden, dev, name, ndc):
    """Row (f1): rays generated on the device vs the reference's dataset code (fixture G10) and the oracle."""
    from mipnerf360_amd.intern import ray as R
    from oracle import ref_path as O
    g = golden("g10_ray_generation")
    n, h, w = (int(x) for x in g["cfg"])
    f, near, far = (float(x) for x in g[name + "_focal_near_far"])
    c2w = g["c2w_ff"] if ndc else g["c2w"]
    rays = R.generate_rays(D(c2w, dev), h, w, f, near, far, ndc)
    for k in synthetic.RAY_FIELDS:
        assert getattr(rays, k).shape == g[f"{name}_{k}"].shape
        close(getattr(rays, k), g[f"{name}_{k}"], atol=2e-7, rtol=4e-5)
    o, d = R.convert_to_ndc(D(g["ndc_in_o"], dev), D(g["ndc_in_d"], dev), 38.25, w, h, 1.0)
    close(o, g["ndc_out_o"], atol=2e-7), close(d, g["ndc_out_d"], atol=2e-7)
    o_np, d_np = R.convert_to_ndc(g["ndc_in_o"], g["ndc_in_d"], 38.25, w, h, 1.0)   # NumPy in -> NumPy out
    assert isinstance(o_np, np.ndarray) and np.allclose(o_np, g["ndc_out_o"], atol=2e-7)
    # a larger, seeded case against the oracle (ragged sizes, one camera given as a single 3x4 pose)
    gen = np.random.Generator(np.random.PCG64(5))
    q, _ = np.linalg.qr(np.eye(3) + 0.1 * gen.normal(size=(3, 3)))
    pose = np.concatenate([q, gen.normal(size=(3, 1))], 1).astype(np.float32)
    if pose[2, 2] < 0:
        pose[:, 2] *= -1
    ro = O.generate_rays(pose[None], 67, 131, 210.0, near, far, ndc)
    rd = R.generate_rays(D(pose, dev), 67, 131, 210.0, near, far, ndc)
    for k in synthetic.RAY_FIELDS:
        close(getattr(rd, k), ro[k], atol=2e-7, rtol=1e-4)
    with pytest.raises(RuntimeError):
        R.generate_rays(D(pose, dev), 2, 131, 210.0, near, far, ndc)


def test_render_view_matches_render_image(dev):
    """Pose in -> frame out with rays generated on the device == render_image on host-generated rays."""
    from mipnerf360_amd.intern.ray import Rays
    from oracle import ref_path as O
    h, w, n = 21, 30, 16
    m = build_model(synthetic.make_state_dict(32, 64, seed=4), dev, n, 32, 64, False)
    gen = np.random.Generator(np.random.PCG64(9))
    q, _ = np.linalg.qr(np.eye(3) + 0.1 * gen.normal(size=(3, 3)))
    pose = np.concatenate([q, gen.normal(size=(3, 1)) * 0.1], 1).astype(np.float32)
    if pose[2, 2] < 0:
        pose[:, 2] *= -1
    r = O.generate_rays(pose[None], h, w, 40.0, 0.0, 1.0, True)
    rays_cpu = Rays(*[torch.from_numpy(r[k]) for k in synthetic.RAY_FIELDS])
    a = m.render_image(rays_cpu, h, w, chunks=128)
    b = m.render_view(torch.from_numpy(pose), h, w, 40.0, 0.0, 1.0, ndc=True, chunks=128)
    assert np.abs(a[0].astype(int) - b[0].astype(int)).max() <= 1
    close(a[1], b[1], atol=1e-4, rtol=1e-4), close(a[2], b[2], atol=1e-4)


def test_render_image_partial_last_chunk_vs_oracle(dev):
    """chunks that do not divide the ray count: the reference's partition keeps a short last chunk (model.py:262)."""
    from mipnerf360_amd.intern.ray import Rays
    from oracle import ref_path as O
    h, w, n = 50, 37, 24
    sd = synthetic.make_state_dict(32, 32, seed=6)
    m = build_model(sd, dev, n, 32, 32, True)
    r = synthetic.make_rays("lego", h * w, seed=12)
    rays_cpu = Rays(*[torch.from_numpy(r[k]) for k in synthetic.RAY_FIELDS])
    rgb8, dist, acc = m.render_image(rays_cpu, h, w, chunks=512)
    o8, od, oa = O.render_image(O.rays_from_numpy(r), h, w, O.to_torch_state_dict(sd), O.Hyper(num_samples=n, white_bkgd=True), chunks=512)
    assert np.abs(rgb8.astype(int) - o8.astype(int)).max() <= 1 and (rgb8 != o8).mean() < 0.02
    close(acc, oa, atol=RGB_TOL, rtol=0), close(dist, od, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("np_,nf", [(64, 128), (32, 16), (24, 100)])
def test_unequal_sample_counts_extension(dev, np_, nf):
    """BASELINE configs[2] "hierarchical 64+128": proposal and NeRF stages with different sample counts.
    The reference cannot express this (intern/ray.py:147); parity is against the oracle's same extension."""
    from mipnerf360_amd.model import mipNeRF360
    from mipnerf360_amd import ops
    from oracle import ref_path as O
    sd = synthetic.make_state_dict(64, 128, seed=11)
    r = synthetic.make_rays("garden", 200, seed=13)
    m = mipNeRF360(num_samples=np_, hidden_proposal=64, hidden_nerf=128, device=dev, num_samples_fine=nf)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    rays = dev_rays(r, dev)
    rgb, dist, acc = m(rays)
    assert m.nerf_net.t_vals.shape == (200, nf + 1) and m.nerf_net.fine_weights.shape == (200, nf)
    hp = O.Hyper(num_samples=np_, num_samples_fine=nf)
    o = O.forward(O.rays_from_numpy(r), O.to_torch_state_dict(sd), hp)
    close_render(rgb, dist, acc, *o)
    # staged API gives the same result
    t_hat, w_hat = m.prop_net.forward(rays)
    assert t_hat.shape == (200, np_ + 1)
    out = m.nerf_net.forward(rays, t_hat, w_hat)
    close(out[0], rgb, atol=1e-6)
    tn = ops.resample_t(t_hat, w_hat, 0.01, num_out=nf + 1)
    close(tn, O.resample_t(t_hat.cpu(), w_hat.cpu(), 0.01, None, nf + 1), atol=8e-6)


@pytest.mark.parametrize("M,n,k,act", [(256 * 5, 256, 64, 1), (256 * 9 + 77, 1024, 1024, 1), (300, 96, 128, 2),
                                        (256 * 40, 768, 256, 0), (1, 64, 64, 2), (256 * 70, 1024, 64, 1),
                                        (256 * 301, 256, 128, 1),      # ping-pong kernel: 2 K-steps, 301 tiles on 256 CUs
                                        (256 * 130, 512, 192, 2),      # odd K-step count: buffer parity across tiles
                                        (256 * 301 + 40, 768, 1152, 1),  # one-wave ring kernel: 18 stages, 903 tiles on 256 CUs + ragged rows
                                        (256 * 33, 256, 384, 0)])      # ... 6 stages, no activation
def test_linear_bf16_against_fp64(dev, M, n, k, act):
    """Opt-in bf16 MLP kernel (persistent LDS-DMA path + generic ragged path): bf16 inputs, fp32 accumulation,
    bf16 output.  Reference = exact product of the SAME bf16-rounded operands in fp64, then rounded to bf16:
    the only admissible deviation is the final rounding (1 bf16 ulp = 2^-8 relative) plus fp32 summation noise."""
    from mipnerf360_amd import ops
    g = torch.Generator().manual_seed(M + n + k)
    x = (torch.rand(M, k, generator=g) * 2 - 1).bfloat16()
    w = ((torch.rand(n, k, generator=g) * 2 - 1) * (6.0 / k) ** 0.5)
    b = torch.rand(n, generator=g) - 0.5
    wp, bp = ops.pack_linear_bf16(w.to(dev), b.to(dev), ops.round_up(n, 64), k)
    assert wp.dtype == torch.bfloat16 and wp.shape == (ops.round_up(n, 64), k)
    y = ops.linear_bf16(x.to(dev), wp, bp, act)
    assert y.dtype == torch.bfloat16
    ref = x.double() @ w.bfloat16().double().T + b.double()
    ref = {0: ref, 1: ref.clamp_min(0), 2: torch.sigmoid(ref)}[act]
    got = y[:, :n].float().cpu().double()
    err = (got - ref).abs()
    assert float((err - 2 ** -8 * ref.abs()).max()) <= 2e-3, float(err.max())
    for _ in range(2):  # repeated launches: no race in the persistent tile hand-over / LDS-staged epilogue
        assert torch.equal(ops.linear_bf16(x.to(dev), wp, bp, act), y)


@pytest.mark.parametrize("kind,B,n,hp,hn,wb", [("garden", 96, 128, 256, 1024, False), ("lego", 130, 64, 64, 128, True),
                                               ("garden", 7, 32, 32, 32, False), ("garden", 1024, 128, 256, 1024, False)])
def test_forward_bf16_mode(dev, kind, B, n, hp, hn, wb):
    """mlp_dtype="bf16" (BASELINE configs[4]): against the oracle emulating bf16 storage (tight) and against the
    fp32 oracle (PSNR / max error of the reduced-precision render, SURVEY.md §8c: no hard gate tighter than 2e-2)."""
    from mipnerf360_amd.model import mipNeRF360
    from oracle import ref_path as O
    sd = synthetic.make_state_dict(hp, hn, seed=5)
    r = synthetic.make_rays(kind, B, seed=8)
    m = mipNeRF360(num_samples=n, hidden_proposal=hp, hidden_nerf=hn, white_bkgd=wb, device=dev, mlp_dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    rgb, dist, acc = m(dev_rays(r, dev))
    sdt = O.to_torch_state_dict(sd)
    emu = O.forward(O.rays_from_numpy(r), sdt, O.Hyper(num_samples=n, white_bkgd=wb, mlp_bf16=True))
    ref = O.forward(O.rays_from_numpy(r), sdt, O.Hyper(num_samples=n, white_bkgd=wb))
    assert float((rgb.detach().cpu() - emu[0]).abs().max()) <= 6e-3 and float((acc.detach().cpu() - emu[2]).abs().max()) <= 6e-3
    rgb, acc = rgb.detach(), acc.detach()
    assert float((rgb.cpu() - ref[0]).abs().max()) <= 2e-2 and float((acc.cpu() - ref[2]).abs().max()) <= 2e-2
    mse = float(((rgb.cpu() - ref[0]) ** 2).mean())
    assert -10 * np.log10(max(mse, 1e-20)) > 45.0  # PSNR of the bf16 render against the fp32 render


def test_g11_visualisation(golden, dev):
    """Row (f2): device versions of intern/pose.py's depth / normal visualisation vs the reference (fixture G11)
    and vs the oracle on a larger seeded map; NumPy in -> NumPy out like the reference."""
    from mipnerf360_amd.intern import pose as P
    from oracle import ref_path as O

    def lut_close(a, b, frac=0.01, step=0.05):
        d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max(-1)
        assert d.max() <= step and (d > 1e-5).mean() <= frac, (d.max(), (d > 1e-5).mean())

    g = golden("g11_visualisation")
    depth, acc = g["depth"], g["acc"]
    close(P.depth_to_normals(depth), g["normals"], atol=2e-6)
    close(P.visualize_normals(depth, acc), g["vis_normals"], atol=1e-5)
    close(P.visualize_normals(depth, None), g["vis_normals_noacc"], atol=1e-5)
    close(P.visualize_normals(g["depth_nan"], acc), g["vis_normals_nan"], atol=1e-5)
    assert P.visualize_normals(depth, acc, scaling=2.0) is None  # the reference falls through for scaling != None
    close(P.sinebow(np.linspace(-0.5, 1.5, 41).astype(np.float32)), g["sinebow"], atol=2e-6)
    lut_close(P.visualize_depth(depth, acc, 2.0, 6.0), g["vis_depth_given"])
    lut_close(P.visualize_depth(depth, acc, 0.0, 1.0), g["vis_depth_auto"])      # near = 0 is falsy -> automatic
    lut_close(P.visualize_depth(depth, None, None, None), g["vis_depth_auto2"])
    lut_close(P.visualize_depth(g["depth_nan"], acc, 2.0, 6.0), g["vis_depth_nan"])
    close(P.visualize_depth(depth, acc, 2.0, 6.0, modulus=0.25), g["vis_depth_mod"], atol=2e-4)
    out = P.visualize_depth(D(depth, dev), D(acc, dev), np.float32(2.0), np.array([6.0]))  # tensors in -> tensor out
    assert isinstance(out, torch.Tensor) and out.shape == depth.shape + (3,)
    gen = np.random.Generator(np.random.PCG64(3))
    big = (2.0 + gen.gamma(2.0, 1.0, size=(301, 517))).astype(np.float32)
    bacc = gen.uniform(0, 1, size=big.shape).astype(np.float32)
    close(P.visualize_normals(big, bacc), O.visualize_normals(big, bacc), atol=2e-5)
    lut_close(P.visualize_depth(big, bacc, None, None), O.visualize_depth(big, bacc, None, None))
    lut_close(P.visualize_depth(big, bacc, ignore_frac=0.03), O.visualize_depth(big, bacc, ignore_frac=0.03))  # 155 617-pixel sort
    # round 5: the sort behind ignore_frac is the build's own (stable LSD radix sort on the keys' order-preserving integer image) - a
    # full-frame-sized map with heavy ties (quantised depths), negative values, -0 / +0, +Inf and NaNs: the chosen planes against numpy's
    # stable argsort + sequential float32 cumsum, exactly
    from mipnerf360_amd import ops
    gen = np.random.Generator(np.random.PCG64(11))
    frame = np.round(gen.normal(3.0, 2.0, size=(822, 1237)) * 16.0).astype(np.float32) / 16.0
    frame[gen.uniform(size=frame.shape) < 0.01] = np.nan
    frame[5, :7] = [0.0, -0.0, np.inf, -3.5, 0.0, -0.0, 1e-30]
    facc = gen.uniform(0, 1, size=frame.shape).astype(np.float32)
    for frac in (0.02, 0.3):
        planes = ops.visualize_depth_ex(D(frame, dev), D(facc, dev), ignore_frac=frac, want="planes").cpu().numpy()
        a = np.where(np.isnan(frame), 0.0, facc).astype(np.float32).reshape(-1)
        order = np.argsort(frame.reshape(-1), kind="stable")
        cum = np.cumsum(a[order], dtype=np.float32)
        keep = frame.reshape(-1)[order][(cum >= cum[-1] * np.float32(frac)) & (cum <= cum[-1] * np.float32(1 - frac))]
        eps = np.finfo(np.float32).eps
        assert planes[0] == np.float32(keep[0] - eps) and planes[1] == np.float32(keep[-1] + eps), (frac, planes, keep[0], keep[-1])
    # end to end: render -> device visualisation -> uint8, as test.py:52-56 does with numpy + to8b
    from mipnerf360_amd.intern.utils import to8b
    img = to8b(P.visualize_depth(big, bacc, 1.0, 20.0))
    assert img.dtype == np.uint8 and img.shape == big.shape + (3,)


def test_rccl_path_single_rank_torchrun(dev):
    """The multi-GPU code path (torch.distributed 'nccl' = RCCL, all_gather_into_tensor of the pixel block) launched
    exactly like the driver launches bench.py, with one rank (the GPU box has one GPU): tools/dist_check.py compares
    the sharded render with the single-process render bit for bit, and bench.py must run under torchrun."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    base = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
            "127.0.0.1", "--master-port"]
    res = subprocess.run(base + ["29541", os.path.join(root, "tools", "dist_check.py")], env=env, cwd=root,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "sharded==single: True" in res.stdout, res.stdout[-2000:]
    assert "forward_sharded max |diff| vs whole-batch forward: 0.00e+00" in res.stdout, res.stdout[-2000:]
    res = subprocess.run(base + ["29542", os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                                 "--cpu-rays", "0", "--full"], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:]
    import json
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 1000 and line["roofline"]["frac"] > 0.5 and line["dtype"] == "f32"


def test_empty_batch(dev):
    m = build_model(synthetic.make_state_dict(32, 32, seed=1), dev, 16, 32, 32, False)
    r = dev_rays(synthetic.make_rays("lego", 0, seed=1), dev)
    rgb, dist, acc = m(r)
    assert rgb.shape == (0, 3) and dist.shape == (0,) and acc.shape == (0,)


def test_repack_after_weight_update(dev):
    """The packed-weight cache must follow load_state_dict / in-place updates."""
    from oracle import ref_path as O
    r = synthetic.make_rays("lego", 16, seed=1)
    m = build_model(synthetic.make_state_dict(32, 64, seed=1), dev, 16, 32, 64, True)
    a = m(dev_rays(r, dev))[0].clone()
    sd2 = synthetic.make_state_dict(32, 64, seed=2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
    b = m(dev_rays(r, dev))[0]
    o = O.forward(O.rays_from_numpy(r), O.to_torch_state_dict(sd2), O.Hyper(num_samples=16, white_bkgd=True))
    assert not torch.equal(a, b)
    close(b, o[0], atol=RGB_TOL, rtol=0)


# ------------------------------------------------------------------ row f3: losses with analytic gradients
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_g12_losses_and_gradients(golden, dev, tag):
    """HIP loss kernels behind the mirrors of intern/loss.py / distillation.py / regularization.py, forward values
    and the gradients autograd receives, against the reference's own values + autograd gradients (G12).
    Tolerance: fp32 sums of up to B*N^2 terms in a different association -> rtol 2e-5."""
    from mipnerf360_amd.intern import distillation, loss
    g = golden("g12_losses")
    t, w, t_hat, s = (D(g[f"{tag}.{k}"], dev) for k in ("t", "w", "t_hat", "s"))
    w_hat = D(g[f"{tag}.w_hat"], dev).requires_grad_(True)
    lp = loss.Loss_prop(t=t, w=w, t_hat=t_hat, w_hat=w_hat)
    lp.backward()
    close(lp, g[f"{tag}.loss_prop"], rtol=2e-5)
    gw = g[f"{tag}.loss_prop.grad_w_hat"]
    close(w_hat.grad, gw, rtol=2e-5, atol=1e-6 * np.abs(gw).max())
    bnd = distillation.bounds(t_vals_fine=t, fine_weights=w, t_vals_coarse=t_hat)
    close(bnd, g[f"{tag}.bounds"], rtol=2e-5)
    assert not bnd.requires_grad and bool((bnd == bnd[:1]).all())      # batch-total quirk of distillation.py:29
    w_hat2 = D(g[f"{tag}.w_hat"], dev).requires_grad_(True)
    lp2 = distillation.loss_prop(coarse_weights=w_hat2, bounds=bnd)
    (3.0 * lp2).backward()                                             # upstream gradient is honoured
    close(lp2, g[f"{tag}.loss_prop_split"], rtol=2e-5)
    close(w_hat2.grad, 3.0 * gw, rtol=2e-5, atol=3e-6 * np.abs(gw).max())

    sv, wv = s.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ld = loss.Loss_dist(s_vals=sv, weights=wv)
    ld.backward()
    close(ld, g[f"{tag}.loss_dist"], rtol=2e-5)
    close(sv.grad, g[f"{tag}.loss_dist.grad_s"], rtol=2e-5, atol=2e-7)
    close(wv.grad, g[f"{tag}.loss_dist.grad_w"], rtol=2e-5, atol=2e-7)

    rgb = D(g[f"{tag}.rgb"], dev).requires_grad_(True)
    ln, psnr = loss.Loss_nerf(input=rgb, target=D(g[f"{tag}.pix"], dev))   # 4-column target: [..., :3] is used
    ln.backward()
    close(ln, g[f"{tag}.loss_nerf"], rtol=2e-5)
    close(psnr, g[f"{tag}.psnr"], rtol=2e-5)
    close(rgb.grad, g[f"{tag}.loss_nerf.grad"], rtol=2e-5, atol=1e-7)
    if tag == "a":
        close(loss.mse_to_psnr(D(g["mse_to_psnr.in"], dev)), g["mse_to_psnr.out"], rtol=1e-6)


def test_losses_training_shape_vs_oracle(dev):
    """BASELINE training shape (4096 rays x 128 intervals): the three losses and their gradients vs the oracle,
    combined the way train.py:75-80 does (loss_nerf + 0.01 * loss_dist, one backward through both)."""
    from mipnerf360_amd.intern import loss
    from oracle import ref_path as O
    gen = np.random.Generator(np.random.PCG64(77))
    B, n = 4096, 128
    t = np.sort(gen.uniform(2, 6, (B, n + 1)), -1).astype(np.float32)
    t_hat = np.sort(gen.uniform(2, 6, (B, n + 1)), -1).astype(np.float32)
    s = np.sort(gen.uniform(0, 1, (B, n + 1)), -1).astype(np.float32)
    w = gen.dirichlet(np.full(n + 1, 0.4), B)[:, :n].astype(np.float32)
    w_hat = gen.dirichlet(np.full(n + 1, 0.6), B)[:, :n].astype(np.float32)
    rgb, pix = gen.uniform(0, 1, (B, 3)).astype(np.float32), gen.uniform(0, 1, (B, 3)).astype(np.float32)
    C = torch.from_numpy

    wh = D(w_hat, dev).requires_grad_(True)
    lp = loss.Loss_prop(D(t, dev), D(w, dev), D(t_hat, dev), wh)
    lp.backward()
    bnd = O.prop_bounds(C(t), C(w), C(t_hat))
    close(lp, O.loss_prop_given(C(w_hat), bnd), rtol=5e-5)
    og = O.loss_prop_grad(C(w_hat), bnd).numpy()
    close(wh.grad, og, rtol=5e-5, atol=1e-6 * np.abs(og).max())

    sv, wv, rv = D(s, dev).requires_grad_(True), D(w, dev).requires_grad_(True), D(rgb, dev).requires_grad_(True)
    ln, _ = loss.Loss_nerf(rv, D(pix, dev))
    ld = loss.Loss_dist(sv, wv)
    (ln + 0.01 * ld).backward()
    close(ld, O.loss_dist(C(s).double(), C(w).double()).float(), rtol=5e-5)
    ogs, ogw = O.loss_dist_grads(C(s).double(), C(w).double())
    close(sv.grad, 0.01 * ogs.float(), rtol=5e-5, atol=1e-8)
    close(wv.grad, 0.01 * ogw.float(), rtol=5e-5, atol=1e-8)
    close(ln, O.loss_nerf(C(rgb), C(pix))[0], rtol=2e-5)
    close(rv.grad, O.loss_nerf_grad(C(rgb), C(pix)), rtol=2e-5, atol=1e-9)


def test_loss_errors_are_loud(dev):
    from mipnerf360_amd import ops
    with pytest.raises(RuntimeError):
        ops.loss_dist(torch.zeros(2, 5), torch.zeros(2, 4))            # CPU tensors
    with pytest.raises(RuntimeError):
        ops.loss_dist(torch.zeros(2, 40001, device=dev), torch.zeros(2, 40000, device=dev))  # exceeds LDS


# ------------------------------------------------------------------ row f3: gradient GEMMs of the MLP
@pytest.mark.parametrize("M,n,k", [(256 * 9, 256, 256), (4096, 1024, 64), (1000, 96, 64), (70, 32, 96), (31, 64, 32),
                                   (256 * 5 + 77, 512, 256)])
def test_linear_wgrad_against_fp64(dev, M, n, k):
    """grad_w = dz^T x and grad_b = colsum(dz) on fp32 MFMA with split rows vs an fp64 matmul.
    Tolerance: fp32 accumulation over M terms -> 2e-6 * sqrt(M) relative to the largest entry; and bitwise
    run-to-run determinism (fixed-order reduction, no atomics)."""
    from mipnerf360_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(M + n + k)
    dz = torch.randn(M, n, generator=gen).to(dev)
    x = torch.randn(M, k, generator=gen).to(dev)
    gw, gb = ops.linear_wgrad(dz, x)
    ref_w = dz.double().t() @ x.double()
    ref_b = dz.double().sum(0)
    tol = 2e-6 * np.sqrt(M)
    assert float((gw.double() - ref_w).abs().max()) <= tol * float(ref_w.abs().max())
    assert float((gb.double() - ref_b).abs().max()) <= tol * float(ref_b.abs().max()) + 1e-6
    gw2, gb2 = ops.linear_wgrad(dz, x)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)


@pytest.mark.parametrize("M,n,k,mask", [(512, 256, 256, True), (300, 64, 96, True), (256 * 3 + 5, 1024, 256, True),
                                        (512, 256, 256, False), (77, 32, 64, False)])
def test_linear_dgrad_against_fp64(dev, M, n, k, mask):
    """dx = (dz W) * [relu_out > 0] through the forward MFMA kernels on the transposed packing."""
    from mipnerf360_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(M * 3 + n + k)
    n_out, k_in = n - 3, k - 5                      # un-padded Linear, zero padding must stay inert
    w = (torch.randn(n_out, k_in, generator=gen) / np.sqrt(n_out)).to(dev)
    dz = torch.randn(M, n, generator=gen).to(dev)
    dz[:, n_out:] = 0
    relu_out = torch.relu(torch.randn(M, k, generator=gen)).to(dev) if mask else None
    wt = ops.pack_linear_transposed(w, n_pad=n, k_pad=k)
    assert torch.equal(wt[:k_in, :n_out], w.t()) and float(wt[k_in:].abs().sum()) == 0 and float(wt[:, n_out:].abs().sum()) == 0
    dx = ops.linear_dgrad(dz, wt, relu_out)
    ref = torch.zeros(M, k, dtype=torch.float64, device=dev)
    ref[:, :k_in] = dz[:, :n_out].double() @ w.double()
    if mask:
        ref = ref * (relu_out > 0)
    close(dx, ref.float(), atol=2e-5, rtol=1e-5)


# ------------------------------------------------------------------ row f3: backward of the two stages
def _grad_close(got, want, name, rel=2e-4):
    """gradient tensors: max |diff| <= rel * max |want| (fp32 sums in a different order than the reference's autograd)"""
    want = H(want) if isinstance(want, torch.Tensor) else np.asarray(want)
    scale = max(float(np.abs(want).max()), 1e-12)
    err = float(np.abs(H(got) - want).max())
    assert err <= rel * scale, f"{name}: max |diff| {err:.3e} > {rel} * {scale:.3e}"


def _g13_model(g, dev, kind):
    B, n, wb = (int(v) for v in g[f"{kind}_cfg"])
    sd = {k[3:]: g[k] for k in g if k.startswith("sd.")}
    m = build_model(sd, dev, n, 32, 64, bool(wb))
    m.train()
    rays = dev_rays({f: g[f"{kind}_rays_{f}"] for f in synthetic.RAY_FIELDS}, dev)
    return m, rays


@pytest.mark.parametrize("kind", ["lego", "garden", "garden70"])
def test_g13_train_step_gradients(golden, dev, kind):
    """The reference's train.py loop body, run UNCHANGED on the mirrors (prop_net.forward / nerf_net.forward / intern.loss
    on the HIP device, loss.backward() through libm360's backward): every parameter gradient vs the reference's autograd
    (G13)."""
    from mipnerf360_amd.intern.loss import Loss_dist, Loss_nerf, Loss_prop
    g = golden("g13_train_gradients")
    model, rays = _g13_model(g, dev, kind)
    # train.py:55-62
    t_hat, w_hat = model.prop_net.forward(rays)
    _, _, _, t, w, _ = model.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    t, w = t.detach(), w.detach()
    loss_prop = Loss_prop(t=t, w=w, t_hat=t_hat, w_hat=w_hat)
    model.zero_grad()
    loss_prop.backward()
    # relu(bounds - w_hat)^2 / (w_hat + 1e-6) divides by weights down to ~1e-6: forward differences of a few 1e-7 in
    # w_hat (the stated forward tolerance) are amplified, hence 5e-4 here instead of the 2e-4 of the other gradients
    close(loss_prop, g[f"{kind}_loss_prop"], rtol=5e-4)
    for name, p in model.named_parameters():
        if name.startswith("prop_net"):
            _grad_close(p.grad, g[f"{kind}_propstep.{name}"], name, rel=5e-4)
        else:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
    # train.py:69-80
    t_hat, w_hat = model.prop_net.forward(rays)
    t_hat, w_hat = t_hat.detach(), w_hat.detach()
    final_rgbs, _, _, _, fine_weights, s_vals = model.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    loss_nerf, psnr = Loss_nerf(input=final_rgbs, target=D(g[f"{kind}_pixels"], dev))
    loss_dist = Loss_dist(s_vals=s_vals, weights=fine_weights)
    loss_all = loss_nerf + 0.01 * loss_dist
    model.zero_grad()
    loss_all.backward()
    close(loss_nerf, g[f"{kind}_loss_nerf"], rtol=5e-5)
    close(loss_dist, g[f"{kind}_loss_dist"], rtol=5e-5)
    for name, p in model.named_parameters():
        if name.startswith("nerf_net"):
            _grad_close(p.grad, g[f"{kind}_nerfstep.{name}"], name)
    # acc path
    model.zero_grad()
    _, _, acc, _, _, _ = model.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    (acc * D(g[f"{kind}_cb"], dev)).sum().backward()
    for name, p in model.named_parameters():
        if name.startswith("nerf_net"):
            _grad_close(p.grad, g[f"{kind}_acc.{name}"], name)


def test_distance_gradient_vs_oracle(golden, dev):
    """d distance / d parameters (the reference raises here, see make_golden.g13): the kernel vs autograd through the oracle."""
    from oracle import ref_path as O
    g = golden("g13_train_gradients")
    kind = "garden"
    model, rays = _g13_model(g, dev, kind)
    B, n, wb = (int(v) for v in g[f"{kind}_cfg"])
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g if k.startswith("sd.")}
    cpu_rays = O.Rays(*[torch.from_numpy(g[f"{kind}_rays_{f}"]) for f in synthetic.RAY_FIELDS])
    ca, cb = g[f"{kind}_ca"], g[f"{kind}_cb"]
    want = O.nerf_output_gradients(cpu_rays, sd, O.Hyper(num_samples=n, white_bkgd=bool(wb)), torch.from_numpy(ca), torch.from_numpy(cb))
    with torch.no_grad():
        t_hat, w_hat = model.prop_net.forward(rays)
    _, dist, acc, _, _, _ = model.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    ((dist * D(ca, dev)).sum() + (acc * D(cb, dev)).sum()).backward()
    for name, p in model.named_parameters():
        if name.startswith("nerf_net"):
            _grad_close(p.grad, want[name], name)


def test_train_step_full_width_vs_oracle(dev):
    """Full-width model (256 / 1024) on a batch the oracle finishes quickly: one AdamW step of each kind on the mirrors
    and on the oracle give the same gradients; exercises the persistent GEMMs, the split-row weight gradient and the
    ragged fallback together (B * N = 2176 rows = 8 full tiles + 128)."""
    from mipnerf360_amd.intern.loss import Loss_dist, Loss_nerf, Loss_prop
    from oracle import ref_path as O
    B, n = 34, 64
    sd_np = synthetic.make_state_dict(256, 1024, seed=3)
    r = synthetic.make_rays("garden", B, seed=5)
    pixels = np.random.Generator(np.random.PCG64(9)).uniform(0, 1, (B, 3)).astype(np.float32)
    model = build_model(sd_np, dev, n, 256, 1024, False).train()
    rays = dev_rays(r, dev)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    cpu_rays = O.Rays(*[torch.from_numpy(r[f]) for f in synthetic.RAY_FIELDS])
    hp = O.Hyper(num_samples=n)

    t_hat, w_hat = model.prop_net.forward(rays)
    _, _, _, t, w, _ = model.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    loss_prop = Loss_prop(t=t.detach(), w=w.detach(), t_hat=t_hat, w_hat=w_hat)
    model.zero_grad()
    loss_prop.backward()
    o_loss, o_grads = O.prop_step_gradients(cpu_rays, sd, hp)
    close(loss_prop, o_loss, rtol=1e-3)       # ill-conditioned loss (division by w_hat + 1e-6), see the G13 test
    for name, p in model.named_parameters():
        if name.startswith("prop_net"):
            _grad_close(p.grad, o_grads[name], name, rel=2e-3)

    model.zero_grad()
    rgb, _, _, _, fw, sv = model.nerf_net.forward(rays, t_vals=t_hat.detach(), coarse_weights=w_hat.detach())
    ln, _ = Loss_nerf(rgb, D(pixels, dev))
    ld = Loss_dist(sv, fw)
    (ln + 0.01 * ld).backward()
    o_ln, o_ld, o_grads = O.nerf_step_gradients(cpu_rays, sd, hp, torch.from_numpy(pixels))
    close(ln, o_ln, rtol=1e-4)
    for name, p in model.named_parameters():
        if name.startswith("nerf_net"):
            _grad_close(p.grad, o_grads[name], name, rel=5e-4)
    # the optimizer of train.py:37 steps the mirrors' parameters like any nn.Module
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    before = model.nerf_net.model[0].weight.detach().clone()
    opt.step()
    assert not torch.equal(before, model.nerf_net.model[0].weight)
    with torch.no_grad():                       # repacked weights are picked up by the next forward
        rgb2, _, _ = model(rays)
    assert not torch.allclose(rgb2, rgb.detach())


@pytest.mark.parametrize("M,n,k,act", [(1024, 256, 64, 1), (2048, 1024, 1024, 1), (700, 256, 256, 2), (300, 96, 64, 0),
                                        (256 * 5 + 77, 512, 128, 1),
                                        (256 * 301 + 9, 768, 192, 1),   # ring kernel: 3 blocks per tile, 903 tiles on 256 CUs + ragged rows
                                        (256 * 20, 256, 320, 0),        # ... 5 blocks, no activation
                                        (256 * 300 + 5, 512, 64, 1)])   # ... one block per tile (the first layers), 600 tiles
def test_linear_bf16x3_against_fp64(dev, M, n, k, act):
    """The bf16x3 layer (m360_linear_bf16x3: [hi | lo] bf16 pair rows in and out, W as [Wh | Wh | Wl]; full tiles of ReLU / plain
    layers with at least two 64-deep blocks on the one-wave ring kernel, sigmoid and 64-deep layers on the 8-wave ping-pong
    kernel - both run xl wh, xh wh, xh wl per block; ragged rows / narrow widths on the generic kernel).  Reference = fp64
    product of the values the pairs REPRESENT (x = hi + lo) with the fp32 weights.  Admissible: the dropped xl wl term
    and the 16-bit representation of w (2^-16 relative each) + the 16-bit representation of the output."""
    from mipnerf360_amd import _lib, ops
    from oracle import ref_path as O
    g = torch.Generator().manual_seed(M + n + k)
    x = torch.rand(M, k, generator=g) * 2 - 1
    w = (torch.rand(n, k, generator=g) * 2 - 1) * (6.0 / k) ** 0.5
    b = torch.rand(n, generator=g) - 0.5
    n_pad = ops.round_up(n, 64)
    wp, bp = ops.pack_linear_bf16x3(w.to(dev), b.to(dev), n_pad, k)
    assert wp.shape == (n_pad, 3 * k) and torch.equal(wp[:, :k], wp[:, k:2 * k])
    xs = ops.split_bf16x3(x.to(dev))
    y = ops.linear_bf16x3(xs, wp, bp, act)
    got = ops.join_bf16x3(y)[:, :n].double().cpu()
    xv = ops.join_bf16x3(xs).double().cpu()
    z = xv @ w.double().t() + b.double()
    ref = torch.relu(z) if act == 1 else (torch.sigmoid(z) if act == 2 else z)
    scale = max(float(ref.abs().max()), 1.0)
    assert float((got - ref).abs().max()) <= 4e-5 * scale, float((got - ref).abs().max())
    # against the oracle's emulation of the same contract (three exact bf16 products, fp32 accumulation): the summation order
    # differs, which can move the LAST bit of the lo term - one unit of the 16-bit pair, 2^-15 of the largest value
    emu = O._lin16x3(xv.float(), {"l.weight": w, "l.bias": b}, "l")
    emu = O._x3(torch.relu(emu) if act == 1 else (torch.sigmoid(emu) if act == 2 else emu)).double()
    assert float((got - emu).abs().max()) <= 2.0 ** -15 * scale
    for _ in range(3):  # a race would not reproduce
        assert torch.equal(ops.linear_bf16x3(xs, wp, bp, act), y)
    # padding columns of a padded width stay zero pairs
    if n_pad > n:
        assert float(ops.join_bf16x3(y)[:, n:].abs().max()) == (0.5 if act == 2 else 0.0)


@pytest.mark.parametrize("kind,n", [("lego", 64), ("garden", 128)])
def test_g8_end_to_end_full_width_bf16x3(golden, dev, kind, n):
    """mlp_dtype="bf16x3" against the REFERENCE's own fp32 outputs (fixture G8, full width): inside the stated fp32
    tolerance (|d rgb|, |d acc| <= 1e-4, |d dist| <= 1e-4 max(1, |dist|)) - the mode keeps 16 significant bits through
    every layer, measured 1e-6-level differences in the rendered values."""
    from mipnerf360_amd.model import mipNeRF360
    g = golden("g8_end_to_end_fullwidth")
    B, n_, wb = (int(x) for x in g[f"{kind}_{n}_cfg"])
    m = mipNeRF360(num_samples=n_, hidden_proposal=256, hidden_nerf=1024, white_bkgd=bool(wb), device=dev, mlp_dtype="bf16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(256, 1024, seed=int(g["weights_seed"][0])).items()})
    rays = dev_rays(synthetic.make_rays(kind, B, seed=int(g["rays_seed"][0])), dev)
    with torch.no_grad():
        rgb, dist, acc = m(rays)
    close_render(rgb, dist, acc, g[f"{kind}_{n}_rgb"], g[f"{kind}_{n}_dist"], g[f"{kind}_{n}_acc"])
    assert float(np.abs(H(rgb) - g[f"{kind}_{n}_rgb"]).max()) <= 2e-5   # what it really achieves, with margin


@pytest.mark.parametrize("kind,B,n,hp,hn,wb", [("garden", 1024, 128, 256, 1024, False), ("lego", 70, 24, 64, 128, True)])
def test_forward_bf16x3_mode(dev, kind, B, n, hp, hn, wb):
    """bf16x3 at the headline shape's width (and at a reduced width with ragged rows: generic kernel) against the fp32
    oracle (1e-4) and against the oracle emulating the mode (tighter); staged == fused; forward only."""
    from mipnerf360_amd.model import mipNeRF360
    from oracle import ref_path as O
    sd = synthetic.make_state_dict(hp, hn, seed=5)
    m = mipNeRF360(num_samples=n, hidden_proposal=hp, hidden_nerf=hn, white_bkgd=wb, device=dev, mlp_dtype="bf16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    r = synthetic.make_rays(kind, B, seed=6)
    rays = dev_rays(r, dev)
    rgb, dist, acc = m(rays)                     # grad enabled: still the forward-only path
    assert not rgb.requires_grad
    t_hat, w_hat = m.prop_net.forward(rays)
    staged = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    assert torch.equal(staged[0], rgb) and torch.equal(staged[2], acc)
    sdt = O.to_torch_state_dict(sd)
    with torch.no_grad():
        ref = O.forward(O.rays_from_numpy(r), sdt, O.Hyper(num_samples=n, white_bkgd=wb))
        emu = O.forward(O.rays_from_numpy(r), sdt, O.Hyper(num_samples=n, white_bkgd=wb, mlp_bf16=2))
    close_render(rgb, dist, acc, ref[0], ref[1], ref[2])
    assert float((rgb.cpu() - emu[0]).abs().max()) <= 1e-5 and float((acc.cpu() - emu[2]).abs().max()) <= 1e-5
    assert float((rgb.cpu() - ref[0]).abs().max()) <= 2e-5


@pytest.mark.parametrize("mode,tol", [("bf16x3", 2e-5), ("bf16", 5e-3)])
def test_reduced_precision_modes_at_the_headline_shape_against_the_fp32_path(dev, mode, tol):
    """BASELINE configs[1] at its full size (4096 rays x 128 samples, 4 x 256 + 8 x 1024 MLPs): every full-tile layer of the opt-in
    precisions runs on the one-wave ring kernel here (32 tiles per CU, single-stage first layers, fused-heads last layers).  The fp32
    HIP path - itself pinned to the CPU oracle at this size - is the reference: bf16x3 must stay inside 2e-5 of it (the fp32
    tolerance is 1e-4), bf16 inside its own 5e-3; finite, deterministic, chunk-independent."""
    from mipnerf360_amd.model import mipNeRF360
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(256, 1024, seed=2).items()}
    rays = dev_rays(synthetic.make_rays("garden", 4096, seed=11), dev)
    outs = {}
    for md in ("fp32", mode):
        m = mipNeRF360(num_samples=128, hidden_proposal=256, hidden_nerf=1024, device=dev, mlp_dtype=md)
        m.load_state_dict(sd)
        m.eval()
        with torch.no_grad():
            outs[md] = m(rays)
            if md == mode:
                again = m(rays)
                assert all(torch.equal(a, b) for a, b in zip(outs[md], again))
        del m
    for a, b in zip(outs[mode], outs["fp32"]):
        assert torch.isfinite(a).all()
    assert float((outs[mode][0] - outs["fp32"][0]).abs().max()) <= tol
    assert float((outs[mode][2] - outs["fp32"][2]).abs().max()) <= tol
    assert float(((outs[mode][1] - outs["fp32"][1]).abs() / outs["fp32"][1].abs().clamp_min(1.0)).max()) <= tol


@pytest.mark.parametrize("gain", [1.0, 4.0, 16.0])
def test_bf16x3_error_does_not_grow_with_the_weight_scale(dev, gain):
    """A trained network is not Kaiming-sized: scale every hidden weight matrix (wider pre-activations, saturating sigmoids,
    larger intermediate values) and the mode's error against the fp32 oracle must stay inside the fp32 tolerance - the split
    keeps 16 significant bits RELATIVE to each value, whatever its size."""
    from mipnerf360_amd.model import mipNeRF360
    from oracle import ref_path as O
    sd = synthetic.make_state_dict(256, 1024, seed=12)
    for k in sd:
        if k.endswith(".weight") and ".model." in k:
            sd[k] = (sd[k] * np.float32(gain ** 0.25)).astype(np.float32)   # 4 / 8 layers deep: the product of gains is what grows
    m = mipNeRF360(num_samples=64, hidden_proposal=256, hidden_nerf=1024, device=dev, mlp_dtype="bf16x3")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    r = synthetic.make_rays("garden", 256, seed=13)
    with torch.no_grad():
        rgb, dist, acc = m(dev_rays(r, dev))
        ref = O.forward(O.rays_from_numpy(r), O.to_torch_state_dict(sd), O.Hyper(num_samples=64))
    close_render(rgb, dist, acc, ref[0], ref[1], ref[2])
    assert float((rgb.cpu() - ref[0]).abs().max()) <= 5e-5


def test_training_bf16_is_forward_only_and_inplace_update_is_caught(golden, dev):
    from mipnerf360_amd.model import mipNeRF360
    g = golden("g13_train_gradients")
    model, rays = _g13_model(g, dev, "lego")
    t_hat, w_hat = model.prop_net.forward(rays)
    with torch.no_grad():
        model.prop_net.model[0].weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        w_hat.sum().backward()
    t2, w2 = model.prop_net.forward(rays)
    w2.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        w2.sum().backward()
    m16 = mipNeRF360(num_samples=16, hidden_proposal=64, hidden_nerf=64, device=dev, mlp_dtype="bf16x3").train()
    t16, w16 = m16.prop_net.forward(rays)      # the bf16x3 MLP is forward-only: no graph, so backward is an error
    assert not w16.requires_grad               # (bf16 trains since round 5: tests/test_gpu_train_bf16.py)
    with pytest.raises(RuntimeError):
        w16.sum().backward()


# ------------------------------------------------------------------ many render_image chunks per launch
@pytest.mark.parametrize("mlp_dtype", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("rays,chunks,super_rays", [(1000, 96, 480), (768, 128, 4096), (300, 7, 64)])
def test_grouped_chunks_bit_identical_to_chunk_loop(dev, rays, chunks, super_rays, mlp_dtype):
    """render_rays launches several of the reference's chunks (model.py:262-264) at once, each with its own contraction
    norm (m360_hyper_t.norm_group_rays).  Must equal the one-launch-per-chunk loop bit for bit, including a ragged last
    chunk and a ragged last super-batch, and must differ from rendering everything as one chunk (the norm is real).
    In the bf16 modes too (their feature rows, first layers and NaN flags ride on the same grouping)."""
    sd = synthetic.make_state_dict(64, 128, seed=11)
    m = _g19_model(sd, dev, 32, 64, 128, False, mlp_dtype)
    r = synthetic.make_rays("garden", rays, seed=12)
    r["origins"] = r["origins"] * 3.0            # push the means outside the unit ball so the norm matters
    m.super_batch_rays = super_rays
    a = [t.clone() for t in m.render_rays(dev_rays(r, dev), chunks)]
    m.super_batch_rays = 0                       # chunks < 0 is never true: one launch sequence per chunk
    b = m.render_rays(dev_rays(r, dev), chunks)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = m.render_rays(dev_rays(r, dev), rays)
    assert not torch.equal(a[0], c[0])


def test_grouped_encode_limits(dev):
    from mipnerf360_amd import _lib
    import ctypes as C
    z = torch.zeros(4096 * 129, device=dev)
    ws = torch.zeros(int(_lib.lib().m360_contract_workspace_bytes()), dtype=torch.uint8, device=dev)
    feat = torch.empty(16, device=dev)
    rc = _lib.lib().m360_encode_features_grouped(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 0, 4096, 128,
                                                 feat.data_ptr(), 64, 0, 2048, ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"131072" in _lib.lib().m360_last_error()


def test_sharded_batch_global_norm_in_process(dev):
    """SURVEY.md §8e opt-in: one batch split into shards that share the contraction norm through a sum of per-shard sums
    of squares (what the all-reduce of distributed.forward_sharded carries).  Emulated in one process: two shards, sums
    added on the device; result vs the whole-batch forward (1e-6: only the summation order of one scalar differs), and
    the sharded result must differ from rendering the shards independently (the norm is real)."""
    sd = synthetic.make_state_dict(64, 128, seed=21)
    m = build_model(sd, dev, 32, 64, 128, True)
    r = synthetic.make_rays("garden", 200, seed=22)
    r["origins"] = r["origins"] * 3.0
    whole = dev_rays(r, dev)
    with torch.no_grad():
        ref = m(whole)
        indep = [m(type(whole)(*[f[a:b] for f in whole])) for a, b in ((0, 120), (120, 200))]
    shards = [type(whole)(*[f[a:b] for f in whole]) for a, b in ((0, 120), (120, 200))]
    t_hat = [m.sharded_sample(s) for s in shards]
    norm = (m.sharded_sumsq(shards[0], t_hat[0]) + m.sharded_sumsq(shards[1], t_hat[1])).sqrt().float()
    t_new = [m.sharded_prop(s, t, norm)[1] for s, t in zip(shards, t_hat)]
    norm2 = (m.sharded_sumsq(shards[0], t_new[0]) + m.sharded_sumsq(shards[1], t_new[1])).sqrt().float()
    outs = [m.sharded_nerf(s, t, norm2) for s, t in zip(shards, t_new)]
    for j in range(3):
        got = torch.cat([o[j] for o in outs], 0)
        close(got, ref[j], atol=2e-6, rtol=2e-6)
    assert float((torch.cat([o[0] for o in indep], 0) - ref[0]).abs().max()) > 1e-4
    # single shard == plain forward, bit for bit (same reduction kernel, same order)
    ss = m.sharded_sumsq(whole, m.sharded_sample(whole))
    w1, t1 = m.sharded_prop(whole, m.sharded_sample(whole), ss.sqrt().float())
    one = m.sharded_nerf(whole, t1, m.sharded_sumsq(whole, t1).sqrt().float())
    for a, b in zip(one, ref):
        assert torch.equal(a, b)


def test_training_descends_end_to_end(dev):
    """tools/train_demo.py: the reference's loop body on the mirrors fits a student to a teacher's pixels; the
    reconstruction PSNR must rise substantially within a few dozen AdamW steps (forward, losses, backward, update all on
    the HIP path)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import train_demo
    out = train_demo.run(steps=40, rays_n=512, samples=16, hp=32, hn=64, lr=3e-3, log_every=39)
    first, last = out["trajectory"][0]["psnr"], out["trajectory"][-1]["psnr"]
    assert np.isfinite(last) and last > first + 3.0, out
    # train.py's default: randomized sampling in both stages (uniforms drawn on the device, consumed by the kernels)
    out = train_demo.run(steps=40, rays_n=512, samples=16, hp=32, hn=64, lr=3e-3, log_every=39, randomized=True)
    first, last = out["trajectory"][0]["psnr"], out["trajectory"][-1]["psnr"]
    assert np.isfinite(last) and last > first + 3.0, out


def test_sample_count_beyond_lds_is_a_loud_error(dev):
    """The per-ray kernels keep one ray's samples in LDS (64 KiB): a sample count that does not fit is refused with an
    error that says so, never truncated."""
    sd = synthetic.make_state_dict(32, 32, seed=5)
    m = build_model(sd, dev, 20000, 32, 32, False)
    with pytest.raises(RuntimeError, match="LDS"):
        with torch.no_grad():
            m(dev_rays(synthetic.make_rays("garden", 2, seed=8), dev))


def test_c_abi_without_python(dev, tmp_path):
    """examples/forward_c_abi.cpp: a plain C++ program (HIP runtime + include/m360.h, no Python / torch) packs weights and
    runs m360_forward; its dump must match the Python mirror fed the same weights and rays, bit for bit (same library,
    same kernels, same launch sequence)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, dump = str(tmp_path / "forward_c_abi"), str(tmp_path / "dump.bin")
    libdir = os.path.join(root, "mipnerf360_amd")
    res = subprocess.run([hipcc, "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "forward_c_abi.cpp"),
                          "-L", libdir, "-lm360", f"-Wl,-rpath,{libdir}", "-o", exe], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    res = subprocess.run([exe, dump, "200", "32", "64", "128"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=300)
    assert res.returncode == 0 and "forward_c_abi:" in res.stdout, res.stdout[-3000:]
    raw = np.fromfile(dump, dtype=np.uint8)
    pos = 0

    def take(count, dtype=np.float32):
        nonlocal pos
        a = raw[pos:pos + 4 * count].view(dtype).copy()
        pos += 4 * count
        return a

    B, N, hp, hn, nl = (int(v) for v in take(5, np.int32))
    names = [f"prop_net.model.{i}" for i in (0, 2, 4, 6, 8)] + [f"nerf_net.model.{i}" for i in range(0, 16, 2)] + \
            ["nerf_net.final_density.0", "nerf_net.final_color.0"]
    assert nl == len(names)
    sd = {}
    for name in names:
        n_out, k_in = (int(v) for v in take(2, np.int32))
        sd[name + ".weight"] = take(n_out * k_in).reshape(n_out, k_in)
        sd[name + ".bias"] = take(n_out)
    rays = {"origins": take(3 * B).reshape(B, 3), "directions": take(3 * B).reshape(B, 3), "viewdirs": take(3 * B).reshape(B, 3),
            "radii": take(B).reshape(B, 1), "near": take(B).reshape(B, 1), "far": take(B).reshape(B, 1)}
    c_rgb, c_dist, c_acc = take(3 * B).reshape(B, 3), take(B), take(B)
    assert pos == raw.size
    m = build_model(sd, dev, N, hp, hn, False)
    with torch.no_grad():
        rgb, dist, acc = m(dev_rays(rays, dev))
    assert np.array_equal(H(rgb), c_rgb) and np.array_equal(H(dist), c_dist) and np.array_equal(H(acc), c_acc)
    assert np.isfinite(c_rgb).all() and c_rgb.std() > 1e-3


def test_bf16_pingpong_kernel_race_screen(dev):
    """The bf16 layer kernels (one-wave ring kernel for ReLU layers with K a multiple of 128, ping-pong kernel otherwise) order
    LDS-DMA, reads and re-staging by counted vmcnt + barriers only; a misplaced read would show as rare wrong tiles.  Screen: 60
    back-to-back launches at the BASELINE layer shape (ring kernel), a small odd one (ping-pong kernel) and a small one with uneven
    tile counts (ring kernel) must all be bit-identical, and agree with an fp64 product of the same bf16 operands to bf16 rounding
    (EVERY row of the small shapes, a strided row sample of the big one)."""
    from mipnerf360_amd import _lib, ops
    gen = torch.Generator(device="cpu").manual_seed(5)
    for M, n, k in ((4096 * 128, 1024, 1024), (256 * 37, 768, 192), (256 * 111, 768, 384)):
        x = (torch.rand(M, k, generator=gen) * 2 - 1).bfloat16().to(dev)
        w = ((torch.rand(n, k, generator=gen) * 2 - 1) * (6.0 / k) ** 0.5).to(dev)
        b = (torch.rand(n, generator=gen) - 0.5).to(dev)
        wp, bp = ops.pack_linear_bf16(w, b, n, k)
        first = ops.linear_bf16(x, wp, bp, _lib.ACT_RELU)
        out = torch.empty_like(first)
        for _ in range(60):
            ops.linear_bf16(x, wp, bp, _lib.ACT_RELU, out=out)
            assert torch.equal(out, first)
        sub = slice(None, None, 1 if M < 100000 else 97)
        ref = (x[sub].double() @ wp.double().T + bp.double()).clamp_min(0)
        diff = (first[sub].double() - ref).abs()
        assert float(diff.max()) <= 2.0 ** -7 * max(float(ref.abs().max()), 1.0)   # one bf16 rounding of the output


def test_bf16_ring_kernel_is_bitwise_the_pingpong_kernel(dev):
    """Both bf16 layer kernels accumulate the same 32-deep MFMA k-steps in the same order and round once: on the same operands every
    output element must be EQUAL, whatever the tile / stage count and the row strides (tools/diag/w16_soak.py through the diagnostics
    library, which can launch either kernel on any shape; skipped when that library was not built: make -C mipnerf360_amd/csrc diag)."""
    import os
    import subprocess
    import sys
    from mipnerf360_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), "libm360_diag.so")):
        pytest.skip("libm360_diag.so not built")
    # bf16, then bf16x3 (xl wh, xh wh, xh wl per block in both kernels), then both with NaN / Inf / huge / denormal activations planted
    for extra in ([], ["--x3"], ["--special"], ["--x3", "--special"]):
        res = subprocess.run([sys.executable, os.path.join(root, "tools", "diag", "w16_soak.py"), "--shapes", "6", "--seed", "3"] + extra,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-3000:]


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("M,n,k,heads", [(1024, 1024, 1024, 4), (512 + 37, 256, 256, 1), (2048, 512, 128, 4)])
def test_bf16_last_layer_heads_on_the_matrix_pipe(dev, M, n, k, heads, x3):
    """m360_linear_heads_bf16 / _bf16x3: the heads' dot products come out of the layer's own epilogue (MFMAs on the packed
    bf16 row segments x the head rows as two bf16 terms), one partial per row and 32-column piece.  Summed
    over the slots they must equal the product of the layer's STORED activations with the fp32 head rows (to the 16 bits
    the head rows are carried in); with store_y = 0 the fused rows of y stay untouched; tail rows go through y."""
    from mipnerf360_amd import _lib, ops
    g = torch.Generator().manual_seed(M + n + k + heads)
    x = (torch.rand(M, k, generator=g) * 2 - 1).to(dev)
    w = ((torch.rand(n, k, generator=g) * 2 - 1) * (6.0 / k) ** 0.5).to(dev)
    b = (torch.rand(n, generator=g) - 0.5).to(dev)
    hw = ((torch.rand(heads, n, generator=g) * 2 - 1) * (6.0 / n) ** 0.5).to(dev)
    if x3:
        wp, bp = ops.pack_linear_bf16x3(w, b, n, k)
        xs = ops.split_bf16x3(x)
        y_ref = ops.join_bf16x3(ops.linear_bf16x3(xs, wp, bp, _lib.ACT_SIGMOID))
    else:
        wp, bp = ops.pack_linear_bf16(w, b, n, k)
        xs = x.bfloat16()
        y_ref = ops.linear_bf16(xs, wp, bp, _lib.ACT_SIGMOID).float()
    y, part, fused = ops.linear_heads_bf16(xs, wp, bp, hw, store_y=True, x3=x3)
    # store_y = 1 (the tape-keeping forward of the bf16 training path): the plain bf16 form runs on the ring kernel too since round 5 (KEEP_Y)
    ring_keep = (not x3) and k % 128 == 0 and k >= 256
    assert fused == (M // 256) * 256 and part.shape[1] == (2 if ring_keep else 8) * (n // 256)
    y_val = ops.join_bf16x3(y) if x3 else y.float()
    assert torch.equal(y_val, y_ref)                                  # the layer itself is unchanged by the fusion
    want = y_ref[:fused].double() @ hw.double().T                      # [fused, heads]
    got = part.double().sum(1)
    assert float((got - want).abs().max()) <= 3e-5 * max(float(want.abs().max()), 1.0)
    for _ in range(5):  # (40 stores per tile behind counted waits in the KEEP_Y form: the same bits every launch)
        y_again, part_again, _ = ops.linear_heads_bf16(xs, wp, bp, hw, store_y=True, x3=x3)
        assert torch.equal(part_again, part) and torch.equal(y_again, y)
    # store_y = 0 (the rendering forward): layers with a contraction of >= 256 (bf16x3: >= 128) run on the one-wave ring kernel,
    # whose 8 slots per 256 columns are contiguous 32-column pieces (the ping-pong kernel's: 8 of every 16 columns of a 64-column
    # group) - only the sum over the slots is comparable
    y2, part2, _ = ops.linear_heads_bf16(xs, wp, bp, hw, store_y=False, x3=x3)
    ring = (k % 64 == 0 and k >= 128) if x3 else (k % 128 == 0 and k >= 256)
    assert part2.shape[1] == (2 if ring else 8) * (n // 256)   # the ring kernel: one slot per 128-column wave tile
    assert float((part2.double().sum(1) - want).abs().max()) <= 3e-5 * max(float(want.abs().max()), 1.0)
    part = part2
    assert float(y2[:fused].float().abs().max()) == 0.0                # not written
    assert torch.equal(y2[fused:], y[fused:])                          # tail rows: the plain layer, the finisher reads them
    for _ in range(5):
        assert torch.equal(ops.linear_heads_bf16(xs, wp, bp, hw, store_y=False, x3=x3)[1], part)


def test_bf16x3_kernel_race_screen(dev):
    """The same screen for the X3 instantiation of the ping-pong kernel (contraction 3K with the activation column wrapping
    at 2K, split [hi | lo] epilogue with twice the stores and its own counted waits): 40 back-to-back launches at the
    BASELINE layer shape and at a small odd one, every launch bit-identical, every sampled row within the mode's
    accuracy of an fp64 product."""
    from mipnerf360_amd import _lib, ops
    gen = torch.Generator(device="cpu").manual_seed(7)
    for M, n, k in ((4096 * 128, 1024, 1024), (256 * 29, 768, 192)):
        x = (torch.rand(M, k, generator=gen) * 2 - 1).to(dev)
        w = ((torch.rand(n, k, generator=gen) * 2 - 1) * (6.0 / k) ** 0.5).to(dev)
        b = (torch.rand(n, generator=gen) - 0.5).to(dev)
        wp, bp = ops.pack_linear_bf16x3(w, b, n, k)
        xs = ops.split_bf16x3(x)
        first = ops.linear_bf16x3(xs, wp, bp, _lib.ACT_RELU)
        out = torch.empty_like(first)
        for _ in range(40):
            ops.linear_bf16x3(xs, wp, bp, _lib.ACT_RELU, out=out)
            assert torch.equal(out, first)
        sub = slice(None, None, 1 if M < 100000 else 97)
        ref = (ops.join_bf16x3(xs[sub]).double() @ w.double().T + b.double()).clamp_min(0)
        diff = (ops.join_bf16x3(first[sub]).double() - ref).abs()
        assert float(diff.max()) <= 4e-5 * max(float(ref.abs().max()), 1.0)


def test_train_gradients_with_unequal_sample_counts(dev):
    """The num_samples_fine extension ("64+128" style) through the training path: tape and backward are sized by the
    NeRF stage's own sample count; gradients vs autograd through the oracle's same extension."""
    from mipnerf360_amd.intern.loss import Loss_dist, Loss_nerf
    from mipnerf360_amd.model import mipNeRF360
    from oracle import ref_path as O
    B, n, nf = 21, 12, 20
    sd_np = synthetic.make_state_dict(32, 64, seed=31)
    r = synthetic.make_rays("lego", B, seed=32)
    pixels = np.random.Generator(np.random.PCG64(33)).uniform(0, 1, (B, 3)).astype(np.float32)
    m = mipNeRF360(randomized=False, num_samples=n, hidden_proposal=32, hidden_nerf=64, white_bkgd=True, device=dev,
                   num_samples_fine=nf)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()})
    m.train()
    rays = dev_rays(r, dev)
    with torch.no_grad():
        t_hat, w_hat = m.prop_net.forward(rays)
    rgb, _, _, _, fw, sv = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
    assert fw.shape == (B, nf) and sv.shape == (B, nf + 1)
    ln, _ = Loss_nerf(rgb, D(pixels, dev))
    (ln + 0.01 * Loss_dist(sv, fw)).backward()
    hp = O.Hyper(num_samples=n, white_bkgd=True, num_samples_fine=nf)
    cpu_rays = O.Rays(*[torch.from_numpy(r[f]) for f in synthetic.RAY_FIELDS])
    o_ln, _, o_grads = O.nerf_step_gradients(cpu_rays, {k: torch.from_numpy(v) for k, v in sd_np.items()}, hp, torch.from_numpy(pixels))
    close(ln, o_ln, rtol=5e-5)
    for name, p in m.named_parameters():
        if name.startswith("nerf_net"):
            _grad_close(p.grad, o_grads[name], name)


@pytest.mark.parametrize("kind", ["lego", "garden", "mixed"])
@pytest.mark.parametrize("mlp_dtype,limit_db", [("fp32", 1e-3), ("bf16", 0.1), ("bf16x3", 1e-3)])
def test_psnr_within_tenth_db_of_reference(golden, dev, kind, mlp_dtype, limit_db):
    """north_star / SURVEY.md §8c acceptance: 'PSNR within 0.1 dB of reference'.  No dataset exists, so both renders -
    the reference's own and the build's - are scored against the SAME synthetic target image with the standard definition
    -10 log10(mean((a - b)^2)) on [0, 1]; the difference must be <= 0.1 dB.  Since round 4 the renders are those of fixture
    G19 (full width, trained-like weights: rgb std over rays 0.2-0.4, peaked proposal weights, saturated and empty rays) -
    on the near-uniform grey renders of Kaiming weights (fixture G8, rgb std 0.01) there was almost no signal to lose.
    The fp32 path and bf16x3 are held to 1e-3 dB, the opt-in bf16 MLP to the 0.1 dB of the acceptance."""
    from mipnerf360_amd.model import mipNeRF360
    g = golden("g19_structured_weights")
    tag = "full." + kind
    (B, n, wb, hp_, hn_, seed), r, sd = g19_case(g, tag)
    m = mipNeRF360(randomized=False, num_samples=n, hidden_proposal=hp_, hidden_nerf=hn_, white_bkgd=wb, device=dev,
                   mlp_dtype=mlp_dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    with torch.no_grad():
        rgb, _, _ = m(dev_rays(r, dev))
    ref_rgb = g[tag + "_rgb"].astype(np.float64)
    assert ref_rgb.std(0).mean() >= 0.15
    gen = np.random.Generator(np.random.PCG64(808))
    worst = 0.0
    for noise in (0.02, 0.1, 0.3):            # targets from "almost the reference render" (34 dB) to "far from it" (10 dB)
        target = np.clip(ref_rgb + noise * gen.normal(size=ref_rgb.shape), 0.0, 1.0)
        psnr = lambda a: -10.0 * np.log10(np.mean((np.clip(a, 0, 1) - target) ** 2))  # noqa: E731
        worst = max(worst, abs(psnr(H(rgb).astype(np.float64)) - psnr(ref_rgb)))
    print(f"G19 {kind} {mlp_dtype}: PSNR differs from the reference's by {worst:.5f} dB, max |d rgb| {np.abs(H(rgb) - ref_rgb).max():.2e}")
    assert worst <= limit_db, f"PSNR differs from the reference's by {worst:.4f} dB"


def test_generate_rays_span_bit_identical_to_the_full_frame(dev):
    """m360_generate_rays_span (what each rank of a sharded frame render calls for its own block of chunks): any flat
    pixel span equals those rows of the full call bit for bit, pinhole and NDC, spans crossing camera boundaries."""
    from mipnerf360_amd.intern import ray as R
    poses = torch.tensor(np.stack([np.concatenate([np.eye(3), np.array([[0.05 * k], [-0.02], [0.1 + k]])], 1) for k in range(3)]),
                         dtype=torch.float32, device=dev)
    h, w = 17, 23
    for ndc in (False, True):
        near, far = (0.0, 1.0) if ndc else (2.0, 6.0)
        full = R.generate_rays(poses, h, w, 0.9 * w, near, far, ndc)
        for b, e in ((0, 3 * h * w), (0, 1), (5, 5), (100, 391), (h * w - 3, 2 * h * w + 7), (3 * h * w - 1, 3 * h * w)):
            part = R.generate_rays(poses, h, w, 0.9 * w, near, far, ndc, span=(b, e))
            for name, f, p in zip(full._fields, full, part):
                assert p.shape[0] == e - b and torch.equal(p, f[b:e]), (name, b, e, ndc)
    with pytest.raises(RuntimeError):
        R.generate_rays(poses, h, w, 0.9 * w, 0.0, 1.0, True, span=(0, 3 * h * w + 1))


@pytest.mark.parametrize("mlp_dtype", ["fp32", "bf16", "bf16x3"])
def test_full_size_forward_soak_is_deterministic(dev, mlp_dtype):
    """Race screen at the BASELINE shape (4096 x 128, full width): 40 back-to-back forwards must be bit-identical
    (LDS-DMA double buffering, tile hand-over, deferred stores: any ordering bug shows up as sporadic mismatches).  The bf16 modes
    run the ring kernel in five forms per forward (first layer: three-product loop with one term out / x6 with split output, hidden,
    last + heads), the one-launch prologue and the NaN flags."""
    sd = synthetic.make_state_dict(256, 1024, seed=0)
    m = _g19_model(sd, dev, 128, 256, 1024, False, mlp_dtype)
    rays = dev_rays(synthetic.make_rays("garden", 4096, seed=1), dev)
    with torch.no_grad():
        first = [t.clone() for t in m(rays)]
        for _ in range(40):
            out = m(rays)
            assert all(torch.equal(a, b) for a, b in zip(out, first))
    assert bool(torch.isfinite(first[0]).all())


def test_fused_two_stage_and_tape_forwards_are_bit_identical(dev):
    """Three ways through the same kernels must agree bit for bit: the fused driver (m360_forward), the two stage entry
    points called one after the other (prop_net.forward -> nerf_net.forward, what train.py does) and the tape-keeping
    training forward; including a batch with ragged GEMM rows (B * N not a multiple of 256) and full-width layers."""
    for hp, hn, B, n in ((64, 128, 37, 24), (256, 1024, 70, 40)):
        sd = synthetic.make_state_dict(hp, hn, seed=41)
        m = build_model(sd, dev, n, hp, hn, True)
        rays = dev_rays(synthetic.make_rays("lego", B, seed=42), dev)
        with torch.no_grad():
            fused = m(rays)                                             # m360_forward
            t_hat, w_hat = m.prop_net.forward(rays)                     # m360_prop_forward
            staged = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)   # m360_nerf_forward
        t2, w2 = m.prop_net.forward(rays)                               # grad enabled: m360_prop_forward_train
        taped = m.nerf_net.forward(rays, t_vals=t2, coarse_weights=w2)  # m360_nerf_forward_train
        assert w2.requires_grad and taped[0].requires_grad
        assert torch.equal(t_hat, t2) and torch.equal(w_hat, w2.detach())
        for k in range(3):
            assert torch.equal(fused[k], staged[k]) and torch.equal(fused[k], taped[k].detach())
        for k in (3, 4, 5):
            assert torch.equal(staged[k], taped[k].detach())


def test_gradients_are_bitwise_reproducible(dev):
    """Every reduction of the backward (split-row weight gradients, bias / head column sums, loss sums) runs in a fixed
    order without atomics: two backward passes from the same state give bit-identical gradients (full-width model)."""
    from mipnerf360_amd.intern.loss import Loss_dist, Loss_nerf, Loss_prop
    sd = synthetic.make_state_dict(256, 1024, seed=51)
    m = build_model(sd, dev, 48, 256, 1024, False).train()
    rays = dev_rays(synthetic.make_rays("garden", 300, seed=52), dev)
    pixels = torch.rand(300, 3, device=dev)

    def grads():
        m.zero_grad()
        t_hat, w_hat = m.prop_net.forward(rays)
        rgb, _, _, t, w, sv = m.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
        loss = Loss_prop(t=t.detach(), w=w.detach(), t_hat=t_hat, w_hat=w_hat) + Loss_nerf(rgb, pixels)[0] + 0.01 * Loss_dist(sv, w)
        loss.backward()
        return [p.grad.clone() for p in m.parameters()], loss.detach().clone()

    g1, l1 = grads()
    g2, l2 = grads()
    assert torch.equal(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert all(bool(torch.isfinite(a).all()) for a in g1) and any(float(a.abs().max()) > 0 for a in g1)


@pytest.mark.parametrize("kind", ["garden", "lego"])
def test_g14_mutate_like_reference_three_pairs(golden, dev, kind):
    """G14: the loop body of train.py:51-80 on ONE rays object with mutate_like_reference=True - the mirrors bump the
    caller's rays.near / rays.far in place exactly like the reference's g(), so pairs 2 and 3 sample from the drifted
    near / far: every pair's outputs, the gradients of the three steps and the final near / far (bitwise)."""
    from mipnerf360_amd.intern.loss import Loss_dist, Loss_nerf, Loss_prop
    g = golden("g14_mutation")
    B, n, wb = (int(v) for v in g[f"{kind}_cfg"])
    sd = {k[3:]: g[k] for k in g if k.startswith("sd.")}
    model = build_model(sd, dev, n, 32, 64, bool(wb))
    model.train()
    model.set_mutate_like_reference(True)
    rays = dev_rays({f: g[f"{kind}_rays_{f}"] for f in synthetic.RAY_FIELDS}, dev)  # ONE object for the three pairs
    for pair in range(2):
        t_hat, w_hat = model.prop_net.forward(rays)
        _, _, _, t, w, s = model.nerf_net.forward(rays, t_vals=t_hat, coarse_weights=w_hat)
        loss_prop = Loss_prop(t=t.detach(), w=w.detach(), t_hat=t_hat, w_hat=w_hat)
        model.zero_grad()
        loss_prop.backward()
        close(t_hat, g[f"{kind}_p{pair}_t_hat"], atol=0, rtol=3e-6)
        close(w_hat, g[f"{kind}_p{pair}_w_hat"], atol=3e-6)
        close(t, g[f"{kind}_p{pair}_t"], atol=2e-6, rtol=1e-5)
        close(w, g[f"{kind}_p{pair}_w"], atol=3e-6)
        close(s, g[f"{kind}_p{pair}_s"], atol=3e-6)
        assert np.array_equal(H(rays.near), g[f"{kind}_p{pair}_near"]) and np.array_equal(H(rays.far), g[f"{kind}_p{pair}_far"])
        close(loss_prop, g[f"{kind}_p{pair}_loss_prop"], rtol=5e-4)
        for name, p in model.named_parameters():
            if name.startswith("prop_net"):
                _grad_close(p.grad, g[f"{kind}_p{pair}_grad.{name}"], name, rel=5e-4)
    t_hat, w_hat = model.prop_net.forward(rays)
    rgb, dist, acc, t, fine_w, s_vals = model.nerf_net.forward(rays, t_vals=t_hat.detach(), coarse_weights=w_hat.detach())
    loss_nerf, _ = Loss_nerf(input=rgb, target=D(g[f"{kind}_pixels"], dev))
    loss_dist = Loss_dist(s_vals=s_vals, weights=fine_w)
    model.zero_grad()
    (loss_nerf + 0.01 * loss_dist).backward()
    close(t_hat, g[f"{kind}_p2_t_hat"], atol=0, rtol=3e-6)
    close(rgb, g[f"{kind}_p2_rgb"], atol=RGB_TOL), close(acc, g[f"{kind}_p2_acc"], atol=RGB_TOL)
    close(s_vals, g[f"{kind}_p2_s"], atol=3e-6)
    close(loss_nerf, g[f"{kind}_p2_loss_nerf"], rtol=5e-5), close(loss_dist, g[f"{kind}_p2_loss_dist"], rtol=5e-5)
    assert np.array_equal(H(rays.near), g[f"{kind}_p2_near"]) and np.array_equal(H(rays.far), g[f"{kind}_p2_far"])
    for name, p in model.named_parameters():
        if name.startswith("nerf_net"):
            _grad_close(p.grad, g[f"{kind}_p2_grad.{name}"], name)
    # default mode: caller tensors untouched, every pair behaves like the reference's first
    plain = build_model(sd, dev, n, 32, 64, bool(wb))
    fresh = dev_rays({f: g[f"{kind}_rays_{f}"] for f in synthetic.RAY_FIELDS}, dev)
    with torch.no_grad():
        for _ in range(2):
            t0, _ = plain.prop_net.forward(fresh)
            close(t0, g[f"{kind}_p0_t_hat"], atol=0, rtol=3e-6)
    assert np.array_equal(H(fresh.near), g[f"{kind}_rays_near"])


def test_g15_reference_written_checkpoint_loads_and_renders(golden, dev):
    """Row f4: the file the reference's own class wrote with torch.save(model.state_dict()) loads through
    load_reference_checkpoint and renders what the reference rendered (fixture G15)."""
    import os
    from conftest import GOLDEN_DIR
    from mipnerf360_amd import checkpoint
    g = golden("g15_reference_render")
    m = checkpoint.load_reference_checkpoint(os.path.join(GOLDEN_DIR, "g15_reference_checkpoint.pt"), device=dev,
                                             num_samples=int(g["cfg"][0]), white_bkgd=True)
    assert m.hidden_proposal == 16 and m.hidden_nerf == 24 and not m.training
    with torch.no_grad():
        rgb, dist, acc = m(dev_rays({f: g[f"rays_{f}"] for f in synthetic.RAY_FIELDS}, dev))
    close_render(rgb, dist, acc, g["rgb"], g["dist"], g["acc"])
    back = checkpoint.to_reference_state_dict(m)
    ref = torch.load(os.path.join(GOLDEN_DIR, "g15_reference_checkpoint.pt"), map_location="cpu")
    assert list(back) == list(ref) and all(torch.equal(back[k], ref[k]) for k in ref)


def test_g16_diag_lift_and_unstable_moments(golden, dev):
    """gaussian_to_xyz(diag=True) and conical_frustum_to_gaussian(stable=False): public branches of the reference that its
    hot path never takes (fixture G16); diag=True through the contraction raises, as in the reference."""
    from mipnerf360_amd.intern import parameterization as P
    g = golden("g16_dead_branches")
    d, t, radii = D(g["d"], dev), D(g["t"], dev), D(g["radii"], dev)
    mean, cov = P.gaussian_to_xyz(d, D(g["tm"], dev), D(g["tv"], dev), D(g["rv"], dev), diag=True)
    assert cov.shape == g["diag_cov"].shape
    close(mean, g["diag_mean"], atol=1e-7), close(cov, g["diag_cov"], atol=1e-9, rtol=1e-5)
    m, c = P.conical_frustum_to_gaussian(d, t[:, :-1].contiguous(), t[:, 1:].contiguous(), radii, diag=False, stable=False)
    close(m, g["unstable_mean"], atol=1e-6, rtol=1e-5)
    close(c, g["unstable_cov"], atol=2e-3 * float(np.abs(g["unstable_cov"]).max()), rtol=0)
    with pytest.raises(RuntimeError):
        P.conical_frustum_to_gaussian(d, t[:, :-1].contiguous(), t[:, 1:].contiguous(), radii, diag=True)


def _g17_curve(x):
    return 1.0 / (x + np.finfo(np.float32).eps)


def _g17_colormap(v):
    return np.stack([v, 1.0 - v, v * v, np.ones_like(v)], -1)


_G17_CASES = {
    "ignore": dict(depth="depth", acc=True, kw=dict(ignore_frac=0.1)),
    "ignore_nan": dict(depth="depth_nan", acc=True, kw=dict(ignore_frac=0.05)),
    "ignore_noacc_far": dict(depth="depth", acc=False, kw=dict(near=None, far=5.0, ignore_frac=0.2)),
    "curve": dict(depth="depth", acc=True, kw=dict(near=2.0, far=6.0, curve_fn=_g17_curve)),
    "curve_auto": dict(depth="depth", acc=True, kw=dict(curve_fn=_g17_curve, ignore_frac=0.1)),
    "colormap": dict(depth="depth", acc=True, kw=dict(near=2.0, far=6.0, colormap=_g17_colormap)),
    "colormap_mod": dict(depth="depth", acc=True, kw=dict(near=2.0, far=6.0, modulus=0.3, colormap=_g17_colormap)),
    "both": dict(depth="depth", acc=True, kw=dict(curve_fn=_g17_curve, colormap=_g17_colormap, ignore_frac=0.05)),
}


@pytest.mark.parametrize("case", sorted(_G17_CASES))
def test_g17_visualize_depth_options(golden, dev, case):
    """Row f2: visualize_depth with ignore_frac > 0 (device sort + sequential float32 cumsum), a custom curve_fn and a custom
    colormap callable (the caller's host code, applied where the reference applies it) - fixture G17; NumPy in -> NumPy out
    and device tensors in -> device tensor out."""
    from mipnerf360_amd.intern import pose as P
    g = golden("g17_visualize_depth_options")
    c = _G17_CASES[case]
    acc = g["acc"] if c["acc"] else None
    got = P.visualize_depth(g[c["depth"]], acc, **c["kw"])
    assert isinstance(got, np.ndarray) and got.shape == g[case].shape
    # the turbo lookup quantises: a value within 1e-6 of a bin edge may pick the neighbouring entry (<= 1 of 256 steps)
    bad = np.abs(got - g[case]) > 2e-6
    assert bad.mean() < 0.002 and np.abs(got - g[case]).max() < 0.03, (bad.mean(), np.abs(got - g[case]).max())
    dev_out = P.visualize_depth(D(g[c["depth"]], dev), None if acc is None else D(acc, dev), **c["kw"])
    assert isinstance(dev_out, torch.Tensor) and np.array_equal(H(dev_out), got)
