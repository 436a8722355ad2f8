"""The stand-in models of tools/inpaint_fake_model.py for the few-step samplers: the same VAE, tokenizer and text encoder, and a
UNet that also comes with 4 input channels (an ordinary model, as SD-Turbo and the LCM checkpoints are).  A file of its own, so
that the fixtures recorded with inpaint_fake_model.py stay what they are.

FewStepUNet(in_channels=9) computes what FakeUNet computes; with 4 channels the terms of the mask and the masked image's latents
are absent.  Like FakeUNet, nothing in it rounds differently on the two devices: roll, flip, additions and multiplications by
powers of two.
"""
import torch

import inpaint_fake_model as fm


class FewStepUNet(fm.FakeUNet):
    def forward(self, x, t, context=None):
        if self.in_channels == 9:
            return super().forward(x, t, context=context)
        self.count += 1
        ctx = context[:, 0, 0].reshape(-1, 1, 1, 1)
        out = 0.5 * torch.roll(x, 1, dims=-1) - 0.25 * torch.flip(x, dims=[-2])
        out = out + 0.125 * torch.roll(x, 1, dims=1)
        out = out + 0.0625 * ctx + 2.0 ** -12 * t.reshape(-1, 1, 1, 1)
        out = out * self.gain
        if self.record:
            self.inputs.append(x.detach().clone())
            self.outputs.append(out.detach().clone())
            self.pointers.append(x.data_ptr())
        return out


class FewStepModel(fm.FakeInpaintModel):
    def __init__(self, device="cpu", dtype=torch.float32, mean_dtype=None, in_channels=9):
        super().__init__(device, dtype, mean_dtype, in_channels)
        self.unet = FewStepUNet(self.device, dtype, in_channels)
