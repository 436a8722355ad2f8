"""Drop-in for the attention hook of the reference's diffusion_utils.py.

`register_attention_control(model, controller)` (reference diffusion_utils.py:158-292; its one caller is NullInversion.invert,
inversion.py:216, with controller = None): the same UNet lookup, the same walk over the modules whose class is named
`CrossAttention`, the same `place_in_unet` names and layer count.  The forward it installs computes q, k, v with the module's own
linear layers and runs the attention in the fused HIP kernels: under autograd (null-text optimisation differentiates through
every layer, inversion.py:184-212) through engine.differentiable_attention, whose backward recomputes the probabilities from one
saved float per query instead of keeping [(b h), n, n_k] of them; without autograd through engine.stereo_attention.

float16 / bfloat16 q, k, v (null-text optimisation on a half model: the reference casts latents and context to the model's dtype,
model_wrappers.py:306-347): by default they are upcast to float32, run through the float32 kernels and cast back, forward and
backward.  stereo_utils.HALF_ATTENTION = True -- the one switch BNAttention reads too -- sends q, k, v of one half dtype (head
dimension a multiple of 8) to the half kernels instead: under autograd cs_attention_half_fwd_lse / cs_attention_half_bwd
(engine.differentiable_attention(..., native_half=True): no conversion pass, the half tensors and a float32 lse saved for the
backward), without autograd cs_stereo_attention_half.  Anything else keeps the upcast.

The reference hands a controller the [(b h), n, n_k] probabilities, which the fused kernels never form: a controller other than
None is refused with TypeError, an attention mask with ValueError (Stable Diffusion's UNet passes neither).

The replaced forwards are saved the way stereo_utils.register_attention_editor_diffusers saves them: stereo_utils.restore_attention
undoes this hook too, and an editor registered later stacks on top of it.

`diffusion_step`, `diffusion_step_no_cfg`, `init_latent` (reference :29-129): the reference's names, argument order and defaults.
They are a few calls into the caller's UNet and scheduler and run on whatever device the tensors are on; stereodiffusion_nodes.
text2stereoimage builds the Standard mode's loop from them.

No CPU fallback: without a GPU the installed forward raises RuntimeError."""
import torch
import torch.nn as nn

from . import engine, stereo_utils


def _attend(q, k, v, heads, scale):
    """q [(b h), n, d], k and v [(b h), n_k, d] -> [(b), n, h * d] in q's dtype, on the fused kernels."""
    stereo_utils._need_gpu()
    dev = q.device if q.is_cuda else torch.device("cuda", torch.cuda.current_device())
    native_half = bool(stereo_utils.HALF_ATTENTION)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        out = engine.differentiable_attention(q.to(dev), k.to(dev), v.to(dev), heads, scale, native_half=native_half)
    elif (native_half and q.dtype in (torch.float16, torch.bfloat16) and k.dtype == q.dtype and v.dtype == q.dtype
          and q.shape[-1] % 8 == 0):
        qh, kh, vh = (t.detach().to(dev).contiguous() for t in (q, k, v))
        out = engine.stereo_attention(qh, kh, vh, heads, scale, "self")
    else:
        q32, k32, v32 = (t.detach().to(dev, torch.float32).contiguous() for t in (q, k, v))
        out = engine.stereo_attention(q32, k32, v32, heads, scale, "self").to(q.dtype)
    return out if q.is_cuda else out.to(q.device)


def register_attention_control(model, controller):
    """Install the fused attention on every `CrossAttention` module of the model's UNet.  controller must be None (TypeError
    otherwise, before the model is touched)."""
    if controller is not None:
        raise TypeError("register_attention_control: a controller receives the [(b h), n, n_k] attention probabilities, which the "
                        "fused attention never forms; only controller=None (the reference's own use, inversion.py:216) is supported")
    is_comfyui = hasattr(model, 'comfy_model')

    def make_forward(net, place_in_unet):
        scale = net.scale if hasattr(net, 'scale') else net.dim_head ** -0.5

        def attention(x, context, value, mask):
            if mask is not None:
                raise ValueError("the fused attention takes no attention mask")
            source = x if context is None else context
            heads = net.heads

            def split(t):   # [b, n, heads * d] -> [(b heads), n, d]
                b, n, hd = t.shape
                return t.reshape(b, n, heads, hd // heads).permute(0, 2, 1, 3).reshape(b * heads, n, hd // heads)

            q, k = split(net.to_q(x)), split(net.to_k(source))
            v = split(net.to_v(source if value is None else value))
            project = net.to_out[0] if isinstance(net.to_out, nn.ModuleList) else net.to_out
            return project(_attend(q, k, v, heads, float(scale)))

        # the two call conventions differ in their third positional argument, as in the reference (:180, :220)
        if is_comfyui:
            def forward(x, context=None, value=None, mask=None, transformer_options=None, **kwargs):
                return attention(x, context, value, mask)
        else:
            def forward(x, context=None, mask=None, value=None, transformer_options=None, **kwargs):
                return attention(x, context, value, mask)
        return forward

    def walk(net, count, place_in_unet):
        if net.__class__.__name__ == 'CrossAttention':
            if not hasattr(net, stereo_utils._SAVED_FORWARD):
                # an instance attribute shadows the class's forward: remember whether there was one
                setattr(net, stereo_utils._SAVED_FORWARD, net.__dict__.get("forward"))
            net.forward = make_forward(net, place_in_unet)
            return count + 1
        if hasattr(net, 'children'):
            for child in net.children():
                count = walk(child, count, place_in_unet)
        return count

    total = 0
    for name, net in stereo_utils._get_unet(model).named_children():
        if "down" in name or "input" in name:
            total += walk(net, 0, "down")
        elif "up" in name or "output" in name:
            total += walk(net, 0, "up")
        elif "mid" in name:
            total += walk(net, 0, "mid")
    return total


def diffusion_step(model, controller, latents, context, t, guidance_scale, low_resource=False):
    """One denoising step with classifier-free guidance (reference :29-66): context = [unconditional, conditional] embeddings;
    low_resource runs the UNet once per half instead of once on the doubled batch."""
    unet_in = model.scheduler.scale_model_input(latents, t)
    if low_resource:
        uncond = model.unet(unet_in, t, encoder_hidden_states=context[0])["sample"]
        cond = model.unet(unet_in, t, encoder_hidden_states=context[1])["sample"]
    else:
        uncond, cond = model.unet(torch.cat([unet_in, unet_in]), t, encoder_hidden_states=context)["sample"].chunk(2)
    guided = uncond + guidance_scale * (cond - uncond)
    return controller.step_callback(model.scheduler.step(guided, t, latents)["prev_sample"])


def diffusion_step_no_cfg(model, controller, latents, context, t):
    """One denoising step without guidance (reference :69-98): one UNet call on the conditional embeddings alone."""
    unet_in = model.scheduler.scale_model_input(latents, t)
    noise_pred = model.unet(unet_in, t, encoder_hidden_states=context)["sample"]
    return controller.step_callback(model.scheduler.step(noise_pred, t, latents)["prev_sample"])


def init_latent(latent, model, height, width, generator, batch_size):
    """-> (latent, latents): the starting latent [1,C,height/8,width/8] (drawn from `generator` when None is given) and its
    view expanded to batch_size on the model's device (reference :101-129)."""
    channels = model.unet.in_channels
    if latent is None:
        latent = torch.randn((1, channels, height // 8, width // 8), generator=generator)
    return latent, latent.expand(batch_size, channels, height // 8, width // 8).to(model.device)
