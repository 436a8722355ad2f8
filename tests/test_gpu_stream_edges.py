"""The latent-shift, decode and inversion kernels (cs_latentshift.hip, cs_inversion.hip) on the paths their workload never takes:
the plan's descending scan, every exponent mode and a tight reach (tests/golden/stream_edges.npz, the reference's own tables), a
disparity with a NaN or an infinity, the second and third pass of every grid-stride loop, every stage of the loss reduction, every
float16 / bfloat16 input of the DDIM step, and Adam's edges.

Bit for bit: the plan, the shift, the step, the codes.  Within the bound of tests/test_gpu_inversion.py: loss, gradient and Adam --
error(ours, float64) <= max(4 * error(reference in the dtype, float64), one ulp of the dtype at the tensor's largest magnitude),
the reference's error measured here from torch running the reference's expression, never from the kernel."""
import numpy as np
import pytest
import torch

import inversion_oracle as io_
import make_stream_edge_goldens as mk
import standard_oracle as so
from comfystereo_amd import engine, inversion, stereo_utils
from test_standard_surface import bits
from test_stream_edges_surface import load

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "float16", "bfloat16")
PASS = 4096 * 256                      # items of one pass of a grid-stride loop (stream_grid's cap)
N_STRIDE = 2 * PASS + 37               # some threads iterate three times
# (c1, c2, c3, c4) = (sqrt(1 - a_t), sqrt(a_t), sqrt(1 - a_o), sqrt(a_o)) as float32 values, of two timesteps (a prev and a next
# step) and one set made for the edges: 1.5 * e is a tie at e = 1 + one ulp in both half types, and 300 * x0 overflows float16
COEFFS = {
    "prev": [float(np.float32(v)) for v in io_.step_coeffs(0.4689, 0.6381)],
    "next": [float(np.float32(v)) for v in io_.step_coeffs(0.9991, 0.8367)],
    "edge": [1.5, 1.0, 0.75, 300.0],
}


def f64(t):
    return t.detach().cpu().double().numpy()


def within(got, want64, ref_err, dtype_name, what):
    e, b = io_.err(got, want64), io_.bound(ref_err, dtype_name, want64)
    print(what, "error", e, "bound", b, "reference error", ref_err)
    assert e <= b, (what, e, b)


def same_bits(got, want):
    """Bit patterns equal, NaNs equal whatever their payload."""
    g, w = got.detach().cpu(), want.detach().cpu()
    ok = (g.view(torch.int32 if g.dtype == torch.float32 else torch.int16) == w.view(torch.int32 if w.dtype == torch.float32 else torch.int16))
    ok |= g.isnan() & w.isnan()
    return bool(ok.all()), int((~ok).sum())


def ref_step(sample, eps_a, eps_b, guidance, coeffs):
    """The reference's expression (inversion.py:88, :59-64) on tensors of the dtype, the coefficients 0-dim float32 tensors as the
    scheduler's alphas are."""
    c1, c2, c3, c4 = (torch.tensor(c, dtype=torch.float32, device=sample.device) for c in coeffs)
    e = eps_a if eps_b is None else eps_a + guidance * (eps_b - eps_a)
    x0 = (sample - c1 * e) / c2
    return c4 * x0 + c3 * e


def kernel_coeffs(kind, dtype):
    """COEFFS[kind] as NullInversion hands them to the kernels for tensors of `dtype`: torch brings a 0-dim float32 tensor that
    multiplies a half tensor to the tensor's dtype first, a divisor stays float32 (inversion._operand)."""
    c = [torch.tensor(v, dtype=torch.float32) for v in COEFFS[kind]]
    return [inversion._operand(c[0], dtype, True), inversion._operand(c[1], dtype, False), inversion._operand(c[2], dtype, True),
            inversion._operand(c[3], dtype, True)]


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def test_plan_equals_every_table_of_the_fixture():
    z, meta = load()
    holes = ident_rows = hits = 0
    seen = set()
    for c in meta["cases"]:
        if c["kind"] in mk.SPECIAL:
            continue
        d = mk.case_depth(c)
        got = engine.latent_shift_plan(torch.from_numpy(d).cuda(), c["scale_factor"], c["exponent"]).cpu().numpy()
        want = mk.table(z, c)
        assert got.dtype == np.int32 and np.array_equal(got, want), (c["id"], int((got != want).sum()))
        holes += int((got < 0).sum())
        ident_rows += int((got == np.arange(got.shape[-1])).all(-1).sum())
        hits += collisions(d, c["scale_factor"], c["exponent"])
        seen.add((c["scale_factor"] > 0, c["exponent"]))
    assert seen == {(s, e) for s in (True, False) for e in mk.EXPONENTS}
    assert holes > 0 and ident_rows > 0 and hits > 0


def collisions(d, sf, e):
    """Destinations of the row sweep that two or more sources reach."""
    prod, _ = so.shift_products(d, sf, e)
    w = d.shape[-1]
    p64 = prod.astype(np.float64)
    cd = np.arange(w) + np.trunc(np.where(np.isfinite(p64), p64, 2.0 * w)).astype(np.int64)
    srt = np.sort(np.where((cd >= 0) & (cd < w), cd, -1).reshape(-1, w), axis=1)
    dup = (srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)
    return int((dup[:, :1].sum() + (dup[:, 1:] & ~dup[:, :-1]).sum()))     # one per run of equal destinations


@pytest.mark.parametrize("shape,factors", [((3, 33, 257), (8.0, -8.0, 150.0, -150.0)), ((1, 2, 8192), (8.0, -8.0))])
def test_plan_equals_the_restatement_on_larger_shapes(shape, factors):
    d = mk.depth("noise", *shape, seed=shape[2])
    dev = torch.from_numpy(d).cuda()
    holes = hits = 0
    for e in mk.EXPONENTS:
        for sf in factors:
            got = engine.latent_shift_plan(dev, sf, e).cpu().numpy()
            want = so.plan(d, sf, e)
            assert np.array_equal(got, want), (shape, e, sf, int((got != want).sum()))
            holes += int((got < 0).sum())
            hits += collisions(d, sf, e)
    assert holes > 0 and hits > 0


def test_apply_through_the_plan_equals_the_shift_kernel():
    """Two kernels that find the winner differently -- k_latent_shift_plan by scanning, k_stereo_shift by LDS atomics -- on the same
    inputs, every exponent and both signs."""
    b, c, h, w = 2, 3, 33, 130
    d = mk.depth("noise", b, h, w, seed=5)
    dev = torch.from_numpy(d).cuda()
    g = torch.Generator().manual_seed(9)
    left = (torch.randn((b, c, h, w), generator=g).abs() + 0.5).cuda()      # no zero: the mask is where something landed
    holes = hits = still = 0
    for e in mk.EXPONENTS:
        for sf in (8.0, -8.0, 100.0 * (w - 1) / w, -99.9, 0.5):
            src = engine.latent_shift_plan(dev, sf, e)
            right = torch.full_like(left, 7.0)
            mask = torch.full((b, h, w), 7, dtype=torch.uint8, device="cuda")
            engine.latent_shift_apply(left, right, src, mask, "first")
            want = stereo_utils.stereo_shift_torch(left, dev, sf, False, e)
            assert torch.equal(want[:b], left)
            assert np.array_equal(bits(right), bits(want[b:])), (e, sf)
            assert torch.equal(mask.bool(), src >= 0)
            holes += int((src < 0).sum())
            hits += collisions(d, sf, e)
            still += int((src == torch.arange(w, device="cuda")).all(-1).sum())
    assert holes > 0 and hits > 0 and still > 0


def test_a_nan_makes_the_map_flat_and_an_infinite_pixel_leaves_the_row():
    """The reference's min() / max() return NaN when the disparity holds one, its range test fails and nothing moves
    (stereo_utils.py:38-43): both kernels follow it.  With a +inf the reference's range is infinite, the infinite pixel's
    normalised value is NaN and int() of its product raises; the kernels cannot raise: that pixel leaves the row and every other
    one stays (norm 0), which is the fixture's table -- made with an int() that does the same."""
    z, meta = load()
    for c in meta["cases"]:
        if c["kind"] not in mk.SPECIAL:
            continue
        d = mk.case_depth(c)
        dev = torch.from_numpy(d).cuda()
        want = mk.table(z, c)
        got = engine.latent_shift_plan(dev, c["scale_factor"], c["exponent"]).cpu().numpy()
        assert np.array_equal(got, want), (c["id"], got, want)
        b, h, w = d.shape
        payload = torch.arange(1, w + 1, dtype=torch.float32, device="cuda").expand(b, 1, h, w).contiguous()
        # (the right view's scale is -scale_factor, stereo_utils.py:84-86, as in the plan)
        shifted = stereo_utils.stereo_shift_torch(payload, dev, c["scale_factor"], False, c["exponent"])[b:, 0]
        assert np.array_equal(shifted.cpu().numpy().astype(np.int32) - 1, want), c["id"]


# ---- the second and third pass of every grid-stride loop --------------------------------------------------------------------
def randn(n, dtype, seed, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, generator=g, device=device, dtype=torch.float32).to(dtype)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_ddim_step_beyond_two_passes(dtype_name):
    dtype = getattr(torch, dtype_name)
    s, a, b = (randn(N_STRIDE, dtype, k) for k in (1, 2, 3))
    for eps_b, guidance, kind in ((b, 7.5, "prev"), (None, 1.0, "next")):
        want = ref_step(s.cpu(), a.cpu(), None if eps_b is None else eps_b.cpu(), guidance, COEFFS[kind])
        out = engine.ddim_step(s, a, eps_b, guidance, kernel_coeffs(kind, dtype))
        ok, bad = same_bits(out, want)
        assert ok, (dtype_name, kind, bad)
        same = s.clone()
        assert engine.ddim_step(same, a, eps_b, guidance, kernel_coeffs(kind, dtype), out=same) is same
        assert same_bits(same, want)[0], (dtype_name, kind, "in place")


def ref_adam(p0, grads, lr, beta1, beta2, eps, first_step=1, state=None):
    """torch.optim.Adam on CPU tensors of the dtype -> [(param, exp_avg, exp_avg_sq) after every step]."""
    from torch.optim.adam import Adam
    p = p0.clone().requires_grad_(True)
    opt = Adam([p], lr=lr, betas=(beta1, beta2), eps=eps)
    out = []
    for k, g in enumerate(grads):
        p.grad = g.clone()
        if k == 0 and state is not None:
            opt.state[p] = dict(step=torch.tensor(float(first_step - 1)), exp_avg=state[0].clone(), exp_avg_sq=state[1].clone())
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


def adam64(p, m, v, g, lr, k, beta1, beta2, eps):
    """One step of io_.adam's float64 formula from a given state."""
    with np.errstate(all="ignore"):
        m = m + (1 - beta1) * (g - m)
        v = beta2 * v + (1 - beta2) * g * g
        denom = np.sqrt(v) / (1 - beta2 ** k) ** 0.5 + eps
        return p - lr / (1 - beta1 ** k) * m / denom, m, v


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_adam_step_beyond_two_passes(dtype_name):
    dtype = getattr(torch, dtype_name)
    p0 = randn(N_STRIDE, dtype, 11)
    grads = [(randn(N_STRIDE, dtype, 12 + k).float() + torch.sign(randn(N_STRIDE, dtype, 12 + k).float()) * 0.05).to(dtype) for k in range(2)]
    want = io_.adam(f64(p0), [f64(g) for g in grads], 1e-2)
    ref = ref_adam(p0.cpu(), [g.cpu() for g in grads], 1e-2, 0.9, 0.999, 1e-8)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for k, g in enumerate(grads, 1):
        assert engine.adam_step(p, g, m, v, 1e-2, k) is p
        for j, (name, got) in enumerate((("param", p), ("exp_avg", m), ("exp_avg_sq", v))):
            within(f64(got), want[k - 1][j], io_.err(f64(ref[k - 1][j]), want[k - 1][j]), dtype_name, f"{dtype_name} step {k} {name}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_latent_shift_apply_beyond_one_pass(dtype):
    b, c, h, w = 1, 2, 1025, 1024            # 1025 * 1024 pixels: the last row is every thread's second pass
    g = torch.Generator(device="cuda").manual_seed(4)
    disp = torch.randint(0, 256, (b, h, w), generator=g, device="cuda").float() / 255.0
    src = engine.latent_shift_plan(disp, 8.0)
    assert int((src < 0).sum()) > 0 and int((src[:, -1] >= 0).sum()) > 0
    left = randn(b * c * h * w, dtype, 5).reshape(b, c, h, w)
    left[0, 0, -1, src[0, -1].clamp(min=0)[:8].long()] = 0.0     # zeros that land in the last row: holes of the mask
    noise = randn(b * c * h * w, dtype, 6).reshape(b, c, h, w)
    idx = src.clamp(min=0).long()[:, None].expand(b, c, h, w)

    def gathered(x):
        return torch.where((src >= 0)[:, None].expand(b, c, h, w), x.gather(3, idx), torch.zeros_like(x))

    ts = gathered(left)
    want_mask = ts[:, 0] != 0
    for with_noise in (False, True):
        right = torch.full_like(left, 7.0)
        mask = torch.full((b, h, w), 7, dtype=torch.uint8, device="cuda")
        engine.latent_shift_apply(left, right, src, mask, "first", noise=noise if with_noise else None)
        want = torch.where(want_mask[:, None].expand(b, c, h, w), ts, noise) if with_noise else ts
        assert torch.equal(mask, want_mask.to(torch.uint8))
        assert same_bits(right, want)[0], with_noise
        new_left = randn(b * c * h * w, dtype, 7).reshape(b, c, h, w)
        before = right.clone()
        engine.latent_shift_apply(new_left, right, src, mask, "reshift")
        want2 = torch.where(want_mask[:, None].expand(b, c, h, w), gathered(new_left), before)
        assert same_bits(right, want2)[0], (with_noise, "reshift")
        assert not torch.equal(right[:, :, -1], before[:, :, -1])


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_decode_to_codes_beyond_one_pass(dtype_name):
    dtype = getattr(torch, dtype_name)
    n, c, h, w = 1, 3, 1024, 1100
    x = (randn(n * c * h * w, torch.float32, 8) * 0.8).to(dtype).reshape(n, c, h, w)
    got = engine.decode_to_codes(x)
    # torch's own arithmetic on the same values, on the CPU as the reference runs it (stereodiffusion_nodes.py:673-677)
    ref = (x.cpu() / 2 + 0.5).clamp(0, 1).float().numpy()
    ref = (np.nan_to_num(ref, nan=0.0, posinf=1.0, neginf=0.0) * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    assert got.shape == (n, h, w, c) and np.array_equal(got.cpu().numpy(), ref)
    assert len(np.unique(ref[:, -70:])) > 200     # the rows of the second pass hold every kind of code


# ---- the loss reduction's stages ---------------------------------------------------------------------------------------------
def loss_case(n, dtype_name, seed, dev_ref):
    """One null_loss_grad call of n elements against the float64 composition and the reference's expression in the dtype
    (autograd through prev_step and mse_loss, inversion.py:198-201), on the CPU or with dev_ref on the device."""
    dtype = getattr(torch, dtype_name)
    coeffs, guidance, kc = COEFFS["prev"], 7.5, kernel_coeffs("prev", dtype)
    eu, ec, cur, nz = (randn(n, dtype, seed + k) for k in range(4))
    step = engine.ddim_step(cur, eu, ec, guidance, kc)
    prev = (step.double() + 0.1 * nz.double()).to(dtype)
    runs = [engine.null_loss_grad(eu, ec, cur, prev, guidance, kc) for _ in range(3)]
    rec, loss, grad = runs[0]
    assert loss.dtype == torch.float32 and loss.shape == () and grad.dtype == dtype
    assert torch.equal(rec.view(torch.uint8), step.view(torch.uint8)), "rec"
    for r2, l2, g2 in runs[1:]:
        assert torch.equal(l2.view(torch.int32), loss.view(torch.int32)) and torch.equal(g2.view(torch.uint8), grad.view(torch.uint8))
        assert torch.equal(r2.view(torch.uint8), rec.view(torch.uint8))
    # float64 on the device, the formulas of io_.null_loss_grad
    c1, c2, c3, c4 = coeffs
    e64 = eu.double() + guidance * (ec.double() - eu.double())
    diff = c4 * ((cur.double() - c1 * e64) / c2) + c3 * e64 - prev.double()
    loss64 = float((diff * diff).mean())
    grad64 = 2.0 / n * diff * (c3 - c4 * c1 / c2) * (1.0 - guidance)
    where = "cuda" if dev_ref else "cpu"
    reu = eu.to(where).clone().requires_grad_(True)
    rrec = ref_step(cur.to(where), reu, ec.to(where), guidance, coeffs)
    rloss = torch.nn.functional.mse_loss(rrec, prev.to(where))
    rloss.backward()
    within(np.float64(loss.item()), np.float64(loss64), abs(float(rloss.detach()) - loss64), dtype_name, f"{dtype_name} n={n} loss")
    ref_grad_err = float((reu.grad.to("cuda").double() - grad64).abs().max())
    got_err = float((grad.double() - grad64).abs().max())
    b = io_.bound(ref_grad_err, dtype_name, np.float64(grad64.abs().max().item()))
    print(dtype_name, "n", n, "grad error", got_err, "bound", b, "reference error", ref_grad_err)
    assert got_err <= b


@pytest.mark.parametrize("k,r", [(0, 1), (0, 1023), (0, 1025), (1, 1), (2, 7), (32, 5), (1024, 5)])
def test_loss_reduction_stages(k, r):
    n = k * 32768 + r
    for dtype_name in (DTYPES if k < 1024 else ("bfloat16",)):
        loss_case(n, dtype_name, 100 * k + r, dev_ref=k >= 1024)


def test_loss_keeps_what_a_float32_running_sum_drops():
    """float32, 32 * 32768 + 5 elements: the differences of the first workgroup's share are 1e3, all others 1e-3.
    Measured on the CPU for these values, the mean of the squares: float64 31249.85099.  A plain float32 running sum of the same
    squares reaches 32 762 384 000 instead of 32 768 000 000 over the first share alone (the sum outgrows 24 bits) and then drops
    every later square: its mean, 31244.495, lies 5.36 from the float64 value, OUTSIDE the bound of one float32 ulp (1.95e-3).  The
    float64 sum rounded to float32, 31249.8515625, lies 5.7e-4 away, inside.  Both are asserted and printed below.  (In this case
    the kernel's own `lo` words are zero -- its tree adds 2^k * 1e6, exactly -- so it tells a two-sum tree from a running sum, not
    a tree that drops `lo`.)"""
    n = 32 * 32768 + 5
    d = torch.full((n,), 1e-3, dtype=torch.float32)
    d[:32768] = 1e3
    sq = (d * d).numpy()
    exact = float(sq.astype(np.float64).sum() / n)
    run = np.float32(0)
    for x in sq[:32768]:
        run = np.float32(run + x)
    assert np.float32(run + sq[-1]) == run       # every later square is dropped: the rest of the running sum changes nothing
    plain = float(run) / n
    zero = torch.zeros(n, device="cuda")
    rec, loss, grad = engine.null_loss_grad(zero, zero, zero, -d.cuda(), 7.5, COEFFS["prev"])
    assert not rec.any()
    ref = float(torch.nn.functional.mse_loss(torch.zeros(n), -d))
    bound = io_.bound(abs(ref - exact), "float32", exact)
    print("float64", exact, "plain float32 running sum", plain, "float64 sum as float32", float(np.float32(exact)), "kernel", loss.item(),
          "reference", ref, "bound", bound)
    assert abs(plain - exact) > bound and abs(float(np.float32(exact)) - exact) <= bound
    within(np.float64(loss.item()), np.float64(exact), abs(ref - exact), "float32", "two-level loss")


def test_loss_keeps_the_lo_words_of_every_workgroup():
    """An exact expectation, float32, two workgroups of 32 768 elements: every thread's first difference is 1, its other 31 are
    2^-13.  A thread's sum is then the pair (1, 31 * 2^-26) -- each square of 2^-26 is below half an ulp of 1 and goes to `lo`
    whole --, a workgroup's (1024, 31 * 2^-16), and every addition on the way is exact.  The loss is
    float32(2048 + 62 * 2^-16) / 65536 = (2048 + 4 ulp) / 65536: 62 * 2^-16 is 3.875 ulp of 2048.  A final stage that drops the
    workgroups' `lo` words gives 2048 / 65536."""
    n = 2 * 32768
    d = torch.full((n,), 2.0 ** -13, dtype=torch.float32)
    d[(torch.arange(n) % 32768) < 1024] = 1.0
    zero = torch.zeros(n, device="cuda")
    _, loss, _ = engine.null_loss_grad(zero, zero, zero, -d.cuda(), 7.5, COEFFS["prev"])
    want = np.float32(2048.0 + 62.0 * 2.0 ** -16) / np.float32(n)
    assert want == np.float32((2048.0 + 4 * 2.0 ** -12) / n) and want == np.float32((d.double() ** 2).sum().item()) / np.float32(n)
    assert np.float32(loss.item()) == want, (loss.item(), float(want), 2048.0 / n)


# ---- every half input of the step ------------------------------------------------------------------------------------------------
def special_values(dtype):
    fi = torch.finfo(dtype)
    ulp1 = fi.eps
    return torch.tensor([0.0, -0.0, fi.smallest_normal * fi.eps, fi.max, 1.0, -1.0, 1.0 + ulp1, 1.0 + 3 * ulp1, float("inf"), float("-inf"),
                         float("nan"), fi.smallest_normal, -fi.max, 0.5, 3 * fi.smallest_normal * fi.eps, 1e-3], dtype=torch.float64).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_step_on_every_half_input(dtype):
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    sp = special_values(dtype)
    ulp = torch.finfo(dtype).eps
    assert 1.5 * float(sp[6]) - (1.5 + ulp) == ulp / 2        # c1 * e of the "edge" set at e = 1 + ulp: halfway between two values
    sample = every.repeat(len(sp))
    eps_a = sp.repeat_interleave(every.numel())
    eps_b = sp.roll(5).repeat_interleave(every.numel())
    dev = [t.cuda() for t in (sample, eps_a, eps_b)]
    if dtype == torch.float16:
        over = ref_step(torch.tensor([300.0], dtype=dtype), torch.tensor([1.0], dtype=dtype), None, 1.0, COEFFS["edge"])
        assert bool(torch.isinf(over).all())          # c4 * x0 overflows
    for kind, guidance in (("prev", 7.5), ("next", 1.0), ("edge", 7.5)):
        for with_b in (True, False):
            want = ref_step(sample, eps_a, eps_b if with_b else None, guidance, COEFFS[kind])
            got = engine.ddim_step(dev[0], dev[1], dev[2] if with_b else None, guidance, kernel_coeffs(kind, dtype))
            ok, bad = same_bits(got, want)
            assert ok, (dtype, kind, with_b, bad)


def test_step_on_float32_specials_and_random_patterns():
    sp = torch.cat([special_values(torch.float32), special_values(torch.float16).float(), special_values(torch.bfloat16).float()])
    g = torch.Generator().manual_seed(21)
    rnd = torch.randint(-2 ** 31, 2 ** 31, (3, 1 << 20), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    k = len(sp)
    sample = torch.cat([sp.repeat(k), rnd[0]])
    eps_a = torch.cat([sp.repeat_interleave(k), rnd[1]])
    eps_b = torch.cat([sp.roll(7).repeat_interleave(k), rnd[2]])
    dev = [t.cuda() for t in (sample, eps_a, eps_b)]
    for kind, guidance in (("prev", 7.5), ("next", 1.0), ("edge", 7.5)):
        for with_b in (True, False):
            want = ref_step(sample, eps_a, eps_b if with_b else None, guidance, COEFFS[kind])
            got = engine.ddim_step(dev[0], dev[1], dev[2] if with_b else None, guidance, COEFFS[kind])
            ok, bad = same_bits(got, want)
            assert ok, (kind, with_b, bad)


# ---- Adam's edges ------------------------------------------------------------------------------------------------------------
def edge_grads(dtype, count, steps):
    fi = torch.finfo(dtype)
    out = []
    for k in range(steps):
        g = randn(count, torch.float32, 40 + k, device="cpu").double()
        g[k::7] = 0.0                                              # exact zeros (at step 1: v = 0, a division by eps)
        g[3::11] = fi.smallest_normal * fi.eps * (1 + (k % 3))     # subnormals
        g[5::13] = -fi.smallest_normal / 2
        g[6::17] = fi.max if k % 2 == 0 else -fi.max               # the dtype's largest value
        out.append(g.to(dtype))
    return out


def class_of(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_adam_edges(dtype_name):
    dtype = getattr(torch, dtype_name)
    count, lr = 4096, 1e-2
    p0 = randn(count, dtype, 30, device="cpu")
    grads = edge_grads(dtype, count, 5)
    for eps in (1e-8, 0.0):
        for beta1 in (0.9, 0.5, 0.25, 0.0):
            for beta2 in (0.999, 0.0):
                # steps 1, 2, 3 from zero moments, then 10 000 and 10 001 from the state they left (both bias corrections are 1)
                ref = ref_adam(p0, grads[:3], lr, beta1, beta2, eps)
                ref += ref_adam(ref[-1][0], grads[3:], lr, beta1, beta2, eps, first_step=10000, state=ref[-1][1:])
                with np.errstate(all="ignore"):
                    want = io_.adam(f64(p0), [f64(g) for g in grads[:3]], lr, beta1, beta2, eps)
                    st = tuple(f64(t) for t in ref[2])       # the float64 run goes on from the reference's state, as ours does
                    for k, g in zip((10000, 10001), grads[3:]):
                        st = adam64(*st, f64(g), lr, k, beta1, beta2, eps)
                        want.append(st)
                p, m, v = p0.cuda(), torch.zeros(count, dtype=dtype, device="cuda"), torch.zeros(count, dtype=dtype, device="cuda")
                for i, (k, g) in enumerate(zip((1, 2, 3, 10000, 10001), grads)):
                    if k == 10000:   # the same state for both: the comparison of the late steps does not inherit the early ones' error
                        p, m, v = (t.cuda() for t in ref[2])
                        p, m, v = p.clone(), m.clone(), v.clone()
                    engine.adam_step(p, g.cuda(), m, v, lr, k, beta1, beta2, eps)
                    for j, (name, got) in enumerate((("param", p), ("exp_avg", m), ("exp_avg_sq", v))):
                        ours, theirs, w64 = f64(got), f64(ref[i][j]), want[i][j]
                        what = f"{dtype_name} eps {eps} betas {beta1} {beta2} step {k} {name}"
                        assert np.array_equal(class_of(ours), class_of(theirs)), (what, int((class_of(ours) != class_of(theirs)).sum()))
                        ok = (class_of(theirs) == 0) & np.isfinite(w64)
                        assert ok.any()
                        within(ours[ok], w64[ok], io_.err(theirs[ok], w64[ok]), dtype_name, what)
