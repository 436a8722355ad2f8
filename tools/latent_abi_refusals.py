"""The ten C entry points of the latent loops on arguments they must refuse: which return code, which cs_last_error() text
(tests/golden/latent_abi_refusals.json, tests/test_latent_abi_refusals.py).

    python tools/latent_abi_refusals.py > tests/golden/latent_abi_refusals.json      (no GPU needed)

cs_latent_shift_plan, cs_latent_shift_apply, cs_decode_to_codes, cs_ddim_step, cs_null_loss_grad, cs_adam_step,
cs_inpaint_image_prep, cs_inpaint_latent_init, cs_inpaint_plms_step and cs_standard_step each get a good call -- made of fake
pointers 256 MiB apart, which nothing dereferences before a refusal -- spoilt in exactly one way per case: every required pointer
null, every size 0 and -1, the dtypes -1 and 3, unknown ops and kinds, every tensor pointer one byte off in each dtype (float32:
two bytes off as well), src_col, loss and workspace two bytes off, every written tensor laid over the last element of every other
written and every read one, every scalar NaN and +inf, the divisors 0 and 1e-60 (0 as a float), the limits one past their end, a
workspace one byte short, noise with an op that takes none, a shift op without its tables, every PLMS kind without a tensor it needs.

A check an entry point does not make is no case: cs_latent_shift_plan looks at no alignment and no overlap, cs_latent_shift_apply and
cs_decode_to_codes at no extent but the ones listed below, and `out == sample` is cs_ddim_step's in-place form.  A case that is not
refused would launch: run() fails on it, so record and replay where there is no GPU first.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from comfystereo_amd import _native   # noqa: E402

REFUSALS = (_native.CS_EINVAL, _native.CS_EWORKSPACE, _native.CS_ELIMIT)
MIN_CASES = 500
NAN, INF = float("nan"), float("inf")
NULL_LOSS_MAX_COUNT = 32768 * 0x7fffffff   # null_loss_max_count(): a 32-bit grid of 32768-element workgroups


class CorpusError(Exception):
    """A case was not refused before the launch, or the corpus is smaller than MIN_CASES."""


def A(i):
    """Fake tensor i: 256 MiB from its neighbours, aligned for any access."""
    return (i + 1) << 28


def eb(a, key="dtype"):
    return 4 if a[key] == 0 else 2


class Entry:
    """One entry point (or one form of it, `tag`): the good call and what its checks look at.
    required: pointers that must not be null; sizes, dtypes, scalars: argument names; enums: name -> (lowest, highest);
    aligned: pointer -> its element's bytes (a function of the arguments); outs / ins: pointer -> (extent in bytes, element bytes)."""

    def __init__(self, fn, good, tag="", required=(), sizes=(), dtypes=(), enums=None, scalars=(), aligned=None, outs=None, ins=None):
        self.fn, self.good, self.tag = fn, good, tag
        self.required, self.sizes, self.dtypes, self.enums, self.scalars = required, sizes, dtypes, enums or {}, scalars
        self.aligned, self.outs, self.ins = aligned or {}, outs or {}, ins or {}

    def case(self, cid, **over):
        unknown = set(over) - set(self.good)
        assert not unknown, (self.fn, unknown)
        return (self.fn, (self.tag + ": " if self.tag else "") + cid, dict(self.good, **over))

    def cases(self):
        out = [self.case(f"{p} null", **{p: None}) for p in self.required]
        out += [self.case(f"{s} = {v}", **{s: v}) for s in self.sizes for v in (0, -1)]
        out += [self.case(f"{d} = {v}", **{d: v}) for d in self.dtypes for v in (-1, 3)]
        out += [self.case(f"{e} = {v}", **{e: v}) for e, (lo, hi) in self.enums.items() for v in (lo - 1, hi + 1)]
        out += [self.case(f"{s} = {v}", **{s: v}) for s in self.scalars for v in (NAN, INF)]
        for dtype in (0, 1, 2) if self.dtypes else (None,):
            a = dict(self.good, **{d: dtype for d in self.dtypes})
            for p, elem in self.aligned.items():
                for off in range(1, elem(a)):
                    if off <= 2:
                        out.append(self.case(f"{p} {off} byte(s) off" + (f", dtypes {dtype}" if self.dtypes else ""),
                                             **{p: a[p] + off}, **{d: dtype for d in self.dtypes}))
        a = self.good
        extents = {**self.ins, **self.outs}
        for o, (_, elem) in self.outs.items():
            for other, (extent, _) in extents.items():
                if other == o or a[other] is None:
                    continue
                at = a[other] + extent(a) - elem(a)   # o's first element is other's last
                assert at % elem(a) == 0 and extent(a) > 0, (self.fn, o, other)
                out.append(self.case(f"{o} over the last element of {other}", **{o: at}))
        return out


def _bytes(count, elem=eb):
    return (lambda a: count(a) * elem(a)), elem


def _one(a):
    return 1


def _four(a):
    return 4


def entries(L):
    """Every Entry, and the cases no Entry rule makes: [(fn, case id, arguments)]"""
    E, extra = [], []
    # ---- cs_latent_shift_plan: no alignment check, no overlap check
    need = L.cs_latent_shift_plan_workspace_bytes()
    plan = Entry("cs_latent_shift_plan",
                 dict(disp=A(0), b=1, h=2, w=8, scale_factor=8.0, stereo_offset_exponent=1.0, src_col=A(1), workspace=A(2),
                      workspace_bytes=need, stream=None),
                 required=("disp", "src_col", "workspace"), sizes=("b", "h", "w"), scalars=("scale_factor", "stereo_offset_exponent"))
    extra += [plan.case("w = 8193", w=8193), plan.case("b = 65536", b=65536), plan.case("2^31 elements", b=65535, h=8192),
              plan.case("workspace one byte short", workspace_bytes=need - 1)]
    E.append(plan)
    # ---- cs_latent_shift_apply: right against left and noise; the extents of src_col and mask are not looked at
    view = _bytes(lambda a: a["b"] * a["c"] * a["h"] * a["w"])
    apply_ = Entry("cs_latent_shift_apply",
                   dict(left=A(0), right=A(1), src_col=A(2), mask=A(3), noise=A(4), dtype=0, b=1, c=4, h=2, w=8, op=0, stream=None),
                   required=("left", "right", "src_col", "mask"), sizes=("b", "c", "h", "w"), dtypes=("dtype",), enums={"op": (0, 1)},
                   aligned={"left": eb, "right": eb, "noise": eb, "src_col": _four}, outs={"right": view}, ins={"left": view, "noise": view})
    extra += [apply_.case("mask null, op RESHIFT", mask=None, op=1, noise=None)]
    E.append(apply_)
    # ---- cs_decode_to_codes
    count = lambda a: a["n"] * a["c"] * a["h"] * a["w"]   # noqa: E731
    E.append(Entry("cs_decode_to_codes", dict(image=A(0), dtype=0, n=1, c=3, h=2, w=8, codes=A(1), stream=None),
                   required=("image", "codes"), sizes=("n", "c", "h", "w"), dtypes=("dtype",), aligned={"image": eb},
                   outs={"codes": _bytes(count, _one)}, ins={"image": _bytes(count)}))
    # ---- cs_ddim_step (out == sample is its in-place form: no case)
    flat = _bytes(lambda a: a["count"])
    coeffs = dict(guidance=1.5, c1=0.5, c2=0.8, c3=0.3, c4=0.9)
    ddim = Entry("cs_ddim_step", dict(sample=A(0), eps_a=A(1), eps_b=A(2), out=A(3), dtype=0, count=4, **coeffs, stream=None),
                 required=("sample", "eps_a", "out"), sizes=("count",), dtypes=("dtype",), scalars=tuple(coeffs),
                 aligned={k: eb for k in ("sample", "eps_a", "eps_b", "out")}, outs={"out": flat},
                 ins={"sample": flat, "eps_a": flat, "eps_b": flat})
    extra += [ddim.case("c2 = 0", c2=0.0), ddim.case("c2 = 1e-60", c2=1e-60)]
    E.append(ddim)
    # ---- cs_null_loss_grad
    ins4 = ("eps_uncond", "eps_cond", "latent_cur", "latent_prev")
    null = Entry("cs_null_loss_grad",
                 dict(eps_uncond=A(0), eps_cond=A(1), latent_cur=A(2), latent_prev=A(3), rec=A(4), loss=A(5), grad=A(6), dtype=0, count=4,
                      **coeffs, workspace=None, workspace_bytes=0, stream=None),
                 required=ins4 + ("rec", "loss", "grad"), sizes=("count",), dtypes=("dtype",), scalars=tuple(coeffs),
                 aligned={k: eb for k in ins4 + ("rec", "grad")}, outs={"rec": flat, "grad": flat, "loss": (_four, _four)},
                 ins={k: flat for k in ins4})
    big = L.cs_null_loss_workspace_bytes(40000)
    assert big > 0
    extra += [null.case("c2 = 0", c2=0.0), null.case("c2 = 1e-60", c2=1e-60), null.case("loss 2 byte(s) off", loss=A(5) + 2),
              null.case("workspace 2 byte(s) off", workspace=A(7) + 2),
              null.case("count above null_loss_max_count()", count=NULL_LOSS_MAX_COUNT + 1),
              null.case("workspace one byte short", count=40000, workspace=A(7), workspace_bytes=big - 1),
              null.case("workspace null where one is needed", count=40000, workspace=None, workspace_bytes=big)]
    E.append(null)
    # ---- cs_adam_step
    adam = Entry("cs_adam_step",
                 dict(param=A(0), grad=A(1), exp_avg=A(2), exp_avg_sq=A(3), dtype=0, count=4, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8,
                      step=1, stream=None),
                 required=("param", "grad", "exp_avg", "exp_avg_sq"), sizes=("count",), dtypes=("dtype",),
                 scalars=("lr", "beta1", "beta2", "eps"), aligned={k: eb for k in ("param", "grad", "exp_avg", "exp_avg_sq")},
                 outs={k: flat for k in ("param", "exp_avg", "exp_avg_sq")}, ins={"grad": flat})
    extra += [adam.case("step = 0", step=0), adam.case("step = -1", step=-1), adam.case("eps = -1e-8", eps=-1e-8)]
    extra += [adam.case(f"{k} = {v}", **{k: v}) for k in ("beta1", "beta2") for v in (1.0, -0.1)]
    E.append(adam)
    # ---- cs_inpaint_image_prep
    pixels = lambda a: a["n"] * a["h"] * a["w"]   # noqa: E731
    unet_in = _bytes(lambda a: 2 * a["n"] * 9 * a["hl"] * a["wl"])
    planes = _bytes(lambda a: 3 * pixels(a))
    E.append(Entry("cs_inpaint_image_prep",
                   dict(filled=A(0), mask=A(1), n=1, h=4, w=8, hl=2, wl=4, dtype=0, img=A(2), masked=A(3), x=A(4), stream=None),
                   required=("filled", "mask", "img", "masked", "x"), sizes=("n", "h", "w", "hl", "wl"), dtypes=("dtype",),
                   aligned={"img": eb, "masked": eb, "x": eb}, outs={"img": planes, "masked": planes, "x": unet_in},
                   ins={"filled": _bytes(lambda a: 3 * pixels(a), _one), "mask": _bytes(pixels, _one)}))
    # ---- cs_inpaint_latent_init
    lat = lambda a: a["n"] * 4 * a["hl"] * a["wl"]   # noqa: E731
    mb = lambda a: eb(a, "mean_dtype")   # noqa: E731
    E.append(Entry("cs_inpaint_latent_init",
                   dict(mean_img=A(0), mean_masked=A(1), mean_dtype=0, noise=A(2), dtype=0, n=1, hl=2, wl=4, sa=0.8, sb=0.6, x=A(3),
                        img_latent=A(4), decode_in=A(5), stream=None),
                   required=("mean_img", "mean_masked", "x", "img_latent"), sizes=("n", "hl", "wl"), dtypes=("dtype", "mean_dtype"),
                   scalars=("sa", "sb"), aligned={"mean_img": mb, "mean_masked": mb, "noise": eb, "x": eb, "img_latent": eb, "decode_in": eb},
                   outs={"x": unet_in, "img_latent": _bytes(lat), "decode_in": _bytes(lat)},
                   ins={"mean_img": _bytes(lat, mb), "mean_masked": _bytes(lat, mb), "noise": _bytes(lat)}))
    # ---- cs_inpaint_plms_step: a pointer the kind does not use is not looked at, so one form per kind of pointer use
    step = dict(noise_pred=A(0), x=A(1), dtype=0, n=1, hl=2, wl=4, kind=4, guidance=3.0, sc=1.0, da=0.5, denom=0.9, e_out=A(2), e1=A(3),
                e2=A(4), e3=A(5), cur_sample=None, decode_in=A(7), stream=None)
    pred = _bytes(lambda a: 2 * lat(a))
    plms = Entry("cs_inpaint_plms_step", step, required=("noise_pred", "x"), sizes=("n", "hl", "wl"), dtypes=("dtype",),
                 enums={"kind": (0, 4)}, scalars=("guidance", "sc", "da", "denom"),
                 aligned={k: eb for k in ("noise_pred", "x", "e_out", "e1", "e2", "e3", "decode_in")},
                 outs={"x": unet_in, "e_out": _bytes(lat), "decode_in": _bytes(lat)},
                 ins={"noise_pred": pred, "e1": _bytes(lat), "e2": _bytes(lat), "e3": _bytes(lat)})
    extra += [plms.case("denom = 0", denom=0.0), plms.case("denom = 1e-60", denom=1e-60)]
    needs = {0: ("e_out", "cur_sample"), 1: ("cur_sample", "e1"), 2: ("e_out", "e1"), 3: ("e_out", "e1", "e2"), 4: ("e_out", "e1", "e2", "e3")}
    for kind, ptrs in needs.items():
        full = dict(kind=kind, cur_sample=A(6))
        extra += [plms.case(f"kind {kind} without {p}", **dict(full, **{p: None})) for p in ptrs]
    E.append(plms)
    E.append(Entry("cs_inpaint_plms_step", dict(step, kind=0, cur_sample=A(6), e1=None, e2=None, e3=None), tag="kind 0",
                   aligned={k: eb for k in ("noise_pred", "x", "e_out", "cur_sample", "decode_in")}, dtypes=("dtype",),
                   outs={"x": unet_in, "e_out": _bytes(lat), "decode_in": _bytes(lat), "cur_sample": _bytes(lat)}, ins={"noise_pred": pred}))
    E.append(Entry("cs_inpaint_plms_step", dict(step, kind=1, cur_sample=A(6), e_out=None, e2=None, e3=None), tag="kind 1",
                   aligned={k: eb for k in ("noise_pred", "x", "e1", "cur_sample", "decode_in")}, dtypes=("dtype",),
                   outs={"x": unet_in, "decode_in": _bytes(lat)}, ins={"noise_pred": pred, "e1": _bytes(lat), "cur_sample": _bytes(lat)}))
    # ---- cs_standard_step
    view = _bytes(lambda a: a["b"] * a["c"] * a["h"] * a["w"])
    whole = _bytes(lambda a: 4 * a["b"] * a["c"] * a["h"] * a["w"])
    pix = lambda a: a["b"] * a["h"] * a["w"]   # noqa: E731
    std = Entry("cs_standard_step",
                dict(x=A(0), noise_pred=A(1), dtype=0, b=1, c=4, h=2, w=8, **coeffs, op=1, src_col=A(2), mask=A(3), noise=A(4), stream=None),
                required=("x", "noise_pred"), sizes=("b", "c", "h", "w"), dtypes=("dtype",), enums={"op": (0, 2)}, scalars=tuple(coeffs),
                aligned={"x": eb, "noise_pred": eb, "noise": eb, "src_col": _four}, outs={"x": whole, "mask": _bytes(pix, _one)},
                ins={"noise_pred": whole, "src_col": _bytes(pix, _four), "noise": view})
    extra += [std.case("c2 = 0", c2=0.0), std.case("c2 = 1e-60", c2=1e-60), std.case("w = 8193", w=8193),
              std.case("b * h = 2^32", b=65536, h=65536), std.case("c * w = 2^31", c=1 << 18, w=8192),
              std.case("noise with op NONE", op=0), std.case("noise with op RESHIFT", op=2)]
    extra += [std.case(f"op {op} without {p}", op=op, noise=None, **{p: None}) for op in (1, 2) for p in ("src_col", "mask")]
    E.append(std)
    return E, extra


def cases(L):
    E, extra = entries(L)
    out = [c for e in E for c in e.cases()] + extra
    ids = [(fn, cid) for fn, cid, _ in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    order = {fn: i for i, fn in enumerate(dict.fromkeys(fn for fn, _, _ in out))}
    return sorted(out, key=lambda c: order[c[0]])   # (stable: one block per entry point)


def run():
    """[[entry point, case id, return code, cs_last_error()]]; CorpusError if a case gets as far as the launch."""
    L = _native.lib()
    rows, accepted = [], []
    for fn, cid, args in cases(L):
        rc = getattr(L, fn)(*args.values())
        msg = L.cs_last_error().decode("utf-8", "replace")
        (rows if rc in REFUSALS else accepted).append([fn, cid, rc, msg])
    if accepted:
        raise CorpusError("not refused:\n" + "\n".join(f"  {fn}: {cid} ({rc}: {msg})" for fn, cid, rc, msg in accepted))
    if len(rows) < MIN_CASES or len({r[0] for r in rows}) != 10:
        raise CorpusError(f"corpus too small: {len(rows)} cases of {len({r[0] for r in rows})} entry points")
    return rows


def dump(rows, out):
    """Compact JSON: every distinct (return code, message) once in "outcomes", per entry point one line of [case id, index]."""
    outcomes, by_fn = [], {}
    for fn, cid, rc, msg in rows:
        if [rc, msg] not in outcomes:
            outcomes.append([rc, msg])
        by_fn.setdefault(fn, []).append([cid, outcomes.index([rc, msg])])
    enc = lambda v: json.dumps(v, separators=(",", ":"), ensure_ascii=True)   # noqa: E731
    comment = "Recorded from the library as it was before the latent-loop entry points' checks were single-sourced."
    out.write('{"comment":%s,\n"outcomes":%s,\n"cases":{\n' % (enc(comment), enc(outcomes)))
    out.write(",\n".join(f"{enc(fn)}:{enc(c)}" for fn, c in by_fn.items()) + "\n}}\n")


def load(path):
    with open(path) as f:
        golden = json.load(f)
    return [[fn, cid] + golden["outcomes"][i] for fn, c in golden["cases"].items() for cid, i in c]


if __name__ == "__main__":
    try:
        dump(run(), sys.stdout)
    except CorpusError as e:
        sys.exit(str(e))
