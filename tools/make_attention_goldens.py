#!/usr/bin/env python3
"""Fixture of the reference's stereo attention: tests/golden/bn_attention.npz.

Build-machine only, like tools/make_gauss_goldens.py: imports the reference's stereo_utils.py (it needs einops), runs its
BNAttention, register_attention_editor_diffusers and restore_attention on seeded inputs (tools/attention_oracle.case_inputs)
and writes the results as data.

  python tools/make_attention_goldens.py
Layout: `meta` = JSON {cases, defaults, legacy_steps, toy}; arrays per case id.
A committed file holds at most 1 MiB and float noise does not compress, so the fixture records
  * the inputs as seeds (np.random.RandomState streams are frozen) -- every reader regenerates them with case_inputs();
  * of every value case a seeded sample of at most SAMPLE output elements: `idx` (flat indices into [(c s b), n, (h d)]),
    `ref` (the reference in float32 on CPU torch) and `ref64` (its own class on float64 copies) at those indices, and
    e_ref = max |ref - ref64| over the WHOLE output;
  * of every routing case nothing but its seed: this script asserts that the reference returns the targets' v rows bit for
    bit (attention_oracle.routing_expected), which is what the tests compare with.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attention_oracle as ao  # noqa: E402
import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SAMPLE = 2048
SHAPES = [(2, 1, 70, 40), (5, 2, 100, 80), (3, 1, 9, 160), (2, 1, 64, 64), (8, 1, 256, 160)]   # heads, samples, n, d
FLAVOURS = {"cfg_uni": ("uni", 2, True), "cfg_bi": ("bi", 2, True), "nocfg": ("bi", 1, False)}   # mode, chunks, use_cfg


def load_ref():
    spec = importlib.util.spec_from_file_location("ref_stereo_utils", refload.REF + "/stereo_utils.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plan():
    cases, seed = [], 100
    for fl, (mode, chunks, _cfg) in FLAVOURS.items():
        for h, b, n, d in SHAPES:
            cases.append(dict(id=f"value_{fl}_{h}x{b}x{n}x{d}", kind="value", flavour=fl, mode=mode, chunks=chunks, heads=h,
                              samples=b, n=n, n_k=n, d=d, seed=seed))
            seed += 1
    for fl in ("cfg_uni", "cfg_bi"):
        mode, chunks, _ = FLAVOURS[fl]
        cases.append(dict(id=f"sharp_{fl}", kind="sharp", flavour=fl, mode=mode, chunks=chunks, heads=2, samples=1, n=70, n_k=70,
                          d=40, seed=seed, gain=3.0))
        seed += 1
    # the plain path (is_cross, or before start_step): the batch as it is -- 4 "samples" = the 2 x 2 CFG / view entries
    for name, h, n, n_k, d, cross in (("plain_self", 2, 70, 70, 40, False), ("plain_cross77", 2, 70, 77, 40, True),
                                      ("plain_n9", 3, 9, 9, 160, False)):
        cases.append(dict(id=name, kind="plain", flavour="plain", mode="self", chunks=1, heads=h, samples=4, n=n, n_k=n_k, d=d,
                          seed=seed, cross=cross))
        seed += 1
    for mode in ("uni", "bi"):
        for h, b, n in ((2, 2, 70), (3, 1, 9)):
            for d in (40, 64, 80, 160):
                cases.append(dict(id=f"routing_{mode}_{h}x{b}x{n}x{d}", kind="routing", flavour="cfg_" + mode, mode=mode, chunks=2,
                                  heads=h, samples=b, n=n, n_k=n, d=d, seed=seed))
                seed += 1
    # large batches, hundreds of workgroups in flight (n = 70 leaves the third wave of a 4-wave workgroup a partial query tile and
    # the fourth none)
    for mode in ("uni", "bi"):
        for h, b, d in ((8, 16, 40), (8, 16, 80), (8, 8, 160), (8, 8, 64)):      # 512 and 256 (c s b h) entries
            cases.append(dict(id=f"routing_{mode}_{h}x{b}x70x{d}", kind="routing", flavour="cfg_" + mode, mode=mode, chunks=2,
                              heads=h, samples=b, n=70, n_k=70, d=d, seed=seed))
            seed += 1
    for fl, h, b, n, d in (("cfg_uni", 8, 16, 70, 40), ("cfg_bi", 8, 8, 70, 160)):
        mode, chunks, _ = FLAVOURS[fl]
        cases.append(dict(id=f"value_{fl}_{h}x{b}x{n}x{d}", kind="value", flavour=fl, mode=mode, chunks=chunks, heads=h, samples=b,
                          n=n, n_k=n, d=d, seed=seed))
        seed += 1
    return cases


def run_reference(ref, case, q, k, v):
    """The reference's class on torch tensors of q's dtype, fed as its ca_forward feeds it (:236-252)."""
    scale = case["d"] ** -0.5
    sim = torch.einsum('b i d, b j d -> b i j', q, k) * scale
    attn = sim.softmax(dim=-1)
    if case["kind"] == "plain":
        ed = ref.BNAttention(start_step=0 if case["cross"] else 4, direction="uni", use_cfg=True)
        return ed.forward(q, k, v, sim, attn, case["cross"], "mid", case["heads"], scale=scale)
    mode, _chunks, use_cfg = FLAVOURS[case["flavour"]]
    ed = ref.BNAttention(start_step=0, direction=mode, use_cfg=use_cfg)
    return ed.forward(q, k, v, sim, attn, False, "mid", case["heads"], scale=scale)


def main():
    ref = load_ref()
    arrays, cases = {}, []
    for case in plan():
        q, k, v = ao.case_inputs(case)
        tq, tk, tv = (torch.from_numpy(t) for t in (q, k, v))
        with torch.no_grad():
            out = run_reference(ref, case, tq, tk, tv).numpy()
            out64 = run_reference(ref, case, tq.double(), tk.double(), tv.double()).numpy()
        assert out.dtype == np.float32 and out64.dtype == np.float64
        scale = case["d"] ** -0.5
        mine = ao.attention(q, k, v, case["heads"], scale, case["mode"], case["chunks"])
        assert mine.shape == out64.shape and np.abs(mine - out64).max() <= 1e-12, (case["id"], np.abs(mine - out64).max())
        if case["kind"] == "routing":
            want = ao.routing_expected(case, v)
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), case["id"]
            assert np.array_equal(ao.attention(q, k, v, case["heads"], scale, case["mode"], case["chunks"], np.float32), want)
        else:
            rs = np.random.RandomState(case["seed"] + 1)
            idx = np.sort(rs.choice(out.size, min(out.size, SAMPLE), replace=False)).astype(np.int32)
            arrays[case["id"] + "/idx"] = idx
            arrays[case["id"] + "/ref"] = out.reshape(-1)[idx]
            arrays[case["id"] + "/ref64"] = out64.reshape(-1)[idx]
            case["e_ref"] = float(np.abs(out.astype(np.float64) - out64).max())
            case["shape"] = list(out.shape)
        cases.append(case)

    # constructor defaults and step bookkeeping
    defaults = {k_: v_ for k_, v_ in vars(ref.BNAttention()).items()}
    tiny = torch.zeros(2, 1, 4)
    legacy = ref.BNAttention(start_step=10 ** 6)
    legacy_steps = []
    for _ in range(70):
        legacy(tiny, tiny, tiny, None, torch.ones(2, 1, 1), False, "mid", 2, scale=1.0)
        legacy_steps.append([legacy.cur_att_layer, legacy.cur_step])

    # the toy model through the reference's register / restore
    net = ao.toy_model()
    state = {k_: v_.numpy().copy() for k_, v_ in net.state_dict().items()}
    for k_, a in state.items():
        arrays["toy/w/" + k_] = a
    mk = lambda: ref.BNAttention(start_step=ao.TOY["start_step"], total_steps=ao.TOY["steps"], direction="uni", use_cfg=True)  # noqa: E731
    outs, book, layers = ao.toy_run(ao.toy_model(state), ref.register_attention_editor_diffusers, ref.restore_attention, mk())
    outs64, _, _ = ao.toy_run(ao.toy_model(state, torch.float64), ref.register_attention_editor_diffusers, ref.restore_attention,
                              mk(), dtype=torch.float64)
    for i, (o, o64) in enumerate(zip(outs, outs64)):
        arrays[f"toy/ref/{i}"] = o
        arrays[f"toy/ref64/{i}"] = o64
    toy = dict(ao.TOY, book=[list(b) for b in book], num_att_layers=layers,
               e_ref=[float(np.abs(o.astype(np.float64) - o64).max()) for o, o64 in zip(outs, outs64)], weights=sorted(state))
    meta = dict(cases=cases, defaults=defaults, legacy_steps=legacy_steps, toy=toy, sample=SAMPLE, numpy=np.__version__,
                torch=torch.__version__)
    path = os.path.join(OUT, "bn_attention.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    print("bn_attention.npz:", len(cases), "cases,", os.path.getsize(path), "bytes")
    for c in cases:
        if "e_ref" in c:
            print(f"  {c['id']:34s} e_ref {c['e_ref']:.3e}")


if __name__ == "__main__":
    main()
