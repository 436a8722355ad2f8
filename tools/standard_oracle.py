"""NumPy restatement of the kernels behind StereoDiffusion's Standard mode (cs_latent_shift_plan, cs_latent_shift_apply,
cs_decode_to_codes) and of the tensor work around them.  The GPU tests compare the kernels with it exactly; tests/
test_standard_surface.py holds it to the reference's own values in tests/golden/standard_mode.npz.

Reference lines restated: stereo_utils.py:36-45 (_norm_depth), :46-71 (_create_stereo's sweep), :84-86 (the right view's scale);
stereodiffusion_nodes.py:39-47, :249-265 (codes, gray, resizes, disparity), :650-667 (shift, mask, deblur fill, re-shift),
:673-677 (the decoded images' codes), :296-305 (the resizes back and the float outputs).
"""
import numpy as np

F32_EPS = np.finfo(np.float32).eps


def norm_depth(depth):
    """stereo_utils.py:36-45 / stereodiffusion_nodes.py:39-47 on a float32 array: its global min / max."""
    depth = np.asarray(depth, dtype=np.float32)
    mn, mx = depth.min(), depth.max()
    with np.errstate(invalid="ignore"):   # (a NaN anywhere: the comparison fails and the map is flat; an infinity: NaN pixels)
        if mx - mn > F32_EPS:
            return (np.float32(1.0) * (depth - mn)) / (mx - mn)
    return np.zeros(depth.shape, dtype=np.float32)


def shift_products(disp, scale_factor, exponent=1.0):
    """norm(disp) ** e * scale_px of the right view, float32 (stereo_utils.py:54, :63-64, :84-86); torch.pow takes the
    exponents 1, 2 and 0.5 as the identity, the square and the square root; any other exponent is glibc's powf (the checker's
    oracle_powf, as in oracle/stereo_shift_oracle.py), which torch's own pow may leave by one unit in the last place."""
    disp = np.asarray(disp, dtype=np.float32)
    w = disp.shape[-1]
    scale_px = ((-1 * float(scale_factor)) / 100.0) * w
    nd = norm_depth(disp)
    if exponent == 1.0:
        dv = nd
    elif exponent == 0.5:
        dv = np.sqrt(nd)
    elif exponent == 2.0:
        dv = nd * nd
    else:
        dv = _powf(nd, exponent)
    with np.errstate(invalid="ignore", over="ignore"):
        return dv * np.float32(scale_px), scale_px


def _powf(nd, exponent):
    """glibc powf(nd, (float)exponent) element by element, once per distinct value."""
    from oracle import oracle
    L = oracle.lib()
    e32 = float(np.float32(exponent))
    vals, inverse = np.unique(nd.ravel().view(np.uint32), return_inverse=True)
    table = np.array([L.oracle_powf(float(v), e32) for v in vals.view(np.float32)], dtype=np.float32)
    return table[inverse].reshape(nd.shape)


def plan(disp, scale_factor, exponent=1.0):
    """disp float32 [B,H,W] -> src_col int32 [B,H,W]: the source column the sweep of stereo_utils.py:57-69 leaves at every
    destination, -1 where nothing lands."""
    prod, scale_px = shift_products(disp, scale_factor, exponent)
    b, h, w = prod.shape
    p64 = prod.astype(np.float64)
    # int() truncates toward zero (:64); of an infinite or NaN product it raises: here such a pixel leaves the row, as in the kernels
    shift = np.trunc(np.where(np.isfinite(p64), p64, 2.0 * w)).astype(np.int64)
    src = np.full((b, h, w), -1, dtype=np.int32)
    bi, ri = np.meshgrid(np.arange(b), np.arange(h), indexing="ij")
    cols = range(w) if scale_px < 0 else range(w - 1, -1, -1)     # (:59-62): what is written last stays
    for col in cols:
        cd = col + shift[:, :, col]
        ok = (cd >= 0) & (cd < w)
        src[bi[ok], ri[ok], cd[ok]] = col
    return src


def _nonzero(a):
    """`x != 0` of a float array, or of its bit pattern held in an integer array (+-0.0 is zero, a NaN is not)."""
    if np.issubdtype(a.dtype, np.integer):
        bits = 8 * a.dtype.itemsize
        return (a.astype(np.int64) & ((1 << (bits - 1)) - 1)) != 0
    return a != 0


def gather(left, src_col):
    """left [B,C,H,W], src_col [B,H,W] -> the shifted view, 0 in the holes (what stereo_shift_torch(...)[1:] returns)."""
    idx = np.clip(src_col, 0, None).astype(np.int64)[:, None].repeat(left.shape[1], 1)
    out = np.take_along_axis(left, idx, axis=3)
    out[(src_col < 0)[:, None].repeat(left.shape[1], 1)] = 0
    return out


def apply_first(left, src_col, noise=None):
    """stereodiffusion_nodes.py:650-660 -> (right, mask uint8 [B,H,W]).  Arrays of floats, or of their bit patterns as integers
    of the same size: values are only moved."""
    ts = gather(left, src_col)
    mask = _nonzero(ts[:, 0])
    right = ts.copy()
    if noise is not None:
        m = mask[:, None].repeat(left.shape[1], 1)
        right[~m] = noise[~m]
    return right, mask.astype(np.uint8)


def apply_reshift(left, right, src_col, mask):
    """stereodiffusion_nodes.py:663-667 -> right: the freshly shifted view where the stored mask is set."""
    ts = gather(left, src_col)
    m = (mask != 0)[:, None].repeat(left.shape[1], 1)
    out = right.copy()
    out[m] = ts[m]
    return out


def _round_bf16(x64):
    """float64 -> the nearest bfloat16 (ties to even) as float64, for values in bfloat16's normal range, 0, inf and NaN."""
    x64 = np.asarray(x64, dtype=np.float64)
    u = x64.view(np.uint64).copy()
    lsb = (u >> np.uint64(45)) & np.uint64(1)
    r = ((u + np.uint64((1 << 44) - 1) + lsb) >> np.uint64(45)) << np.uint64(45)
    out = r.view(np.float64)
    return np.where(np.isfinite(x64), out, x64)


def _round_to(x64, dtype):
    if dtype == "float32":
        return np.asarray(x64, dtype=np.float64).astype(np.float32).astype(np.float64)
    if dtype == "float16":
        return np.asarray(x64, dtype=np.float64).astype(np.float16).astype(np.float64)
    if dtype == "bfloat16":
        return _round_bf16(x64)
    raise ValueError(dtype)


def decode_to_codes(image, dtype):
    """stereodiffusion_nodes.py:673-677: image [N,C,H,W] (the values of a tensor of type `dtype`, held exactly in a float32 or
    float64 array) -> uint8 [N,H,W,C].  The quotient and the sum are each rounded to `dtype` once (float64 holds both exactly
    before the rounding for every value whose code is not decided by the clamp alone)."""
    x = np.asarray(image, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = _round_to(x / 2, dtype)
        s = _round_to(q + 0.5, dtype)
        s = np.clip(s, 0.0, 1.0)                                   # (a NaN stays one)
        s = np.nan_to_num(s.astype(np.float32), nan=0.0, posinf=1.0, neginf=0.0)
        codes = (s * np.float32(255.0)).astype(np.uint8)
    return np.ascontiguousarray(codes.transpose(0, 2, 3, 1))


def margin(disp, scale_factor, exponent=1.0):
    """The smallest distance of a non-zero shift product from an integer: how far the disparity may move before a truncated
    shift can change."""
    prod, _ = shift_products(disp, scale_factor, exponent)
    p = prod.astype(np.float64)
    p = p[np.isfinite(p) & (p != 0)]
    if p.size == 0:
        return float("inf")
    return float(np.abs(p - np.rint(p)).min())


def image_codes(image):
    """stereodiffusion_nodes.py:50-56: float32 -> uint8, clip(255 * x, 0, 255) truncated."""
    return np.clip(np.float32(255.0) * np.asarray(image, dtype=np.float32), 0, 255).astype(np.uint8)


def disparity_512(depth512_u8):
    """stereodiffusion_nodes.py:263-265: the 512 x 512 gray depth codes -> disp float32 [1,512,512]."""
    return norm_depth(depth512_u8.astype(np.float32) / np.float32(255.0))[None]
