"""The ten C entry points of the latent loops refuse what they refused before their checks were single-sourced, with the same
return code and the same cs_last_error() text: the corpus of tools/latent_abi_refusals.py, recorded from the library as it was
(tests/golden/latent_abi_refusals.json), replayed.  Every case is one fault on fake pointers that nothing dereferences before the
refusal, and none may get as far as a launch (not gpu)."""
import os
import sys

from comfystereo_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import latent_abi_refusals   # noqa: E402

ENTRY_POINTS = ["cs_latent_shift_plan", "cs_latent_shift_apply", "cs_decode_to_codes", "cs_ddim_step", "cs_null_loss_grad",
                "cs_adam_step", "cs_inpaint_image_prep", "cs_inpaint_latent_init", "cs_inpaint_plms_step", "cs_standard_step"]


def test_every_case_is_refused_as_recorded():
    want = latent_abi_refusals.load(os.path.join(ROOT, "tests", "golden", "latent_abi_refusals.json"))
    assert len(want) >= latent_abi_refusals.MIN_CASES and list(dict.fromkeys(row[0] for row in want)) == ENTRY_POINTS
    got = latent_abi_refusals.run()   # (CorpusError if a case is not refused before the launch)
    assert [row[:2] for row in got] == [row[:2] for row in want]
    for g, w in zip(got, want):
        assert g == w
    assert all(row[2] != _native.CS_OK and row[2] in latent_abi_refusals.REFUSALS for row in got)
