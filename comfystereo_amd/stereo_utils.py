"""Drop-in for the reference's stereo_utils.py.

`stereo_shift_torch` (reference stereo_utils.py:15-88; called on diffusion latents by stereodiffusion_nodes.py:650, :664): same
name, argument order, defaults and return shape; the shift runs in a HIP kernel behind the C ABI (cs_stereo_shift).

`BNAttention`, `register_attention_editor_diffusers`, `restore_attention` (reference :91-393), the attention editing of
StereoDiffusion's Standard mode: the same classes, names, signatures and step bookkeeping; the attention itself is one fused
HIP kernel behind the C ABI (cs_stereo_attention) that never materialises the score matrix -- the reference builds
`sim` and `softmax(sim)` twice per layer, [heads, 2n, 2n] float32 the second time.

float16 / bfloat16 q, k, v: by default they are upcast to float32, run through the float32 kernel and the result is cast back
(three conversion passes in, one out, at the f32-input MFMA's rate).  `HALF_ATTENTION = True` (a module switch, like
engine.MESH_WARP / engine.DIALECT) sends them to cs_stereo_attention_half instead, with no conversion pass: the matrix
operands (q, k, v, and the probabilities after the exponential) stay half on the half-input MFMA, the scores, the softmax and
the accumulators are float32 -- the reference's own arithmetic in that dtype rounds more, not less.  float32 inputs take the
float32 kernel either way.  diffusion_utils.register_attention_control reads the same switch: with it set, half q, k, v take
cs_stereo_attention_half without autograd and the half forward-with-lse / backward pair under autograd.

No CPU fallback anywhere: without a GPU the calls raise RuntimeError."""
import torch
import torch.nn as nn

from . import engine


def stereo_shift_torch(input_images: torch.Tensor, depthmaps: torch.Tensor, scale_factor: float = 8.0,
                       shift_both: bool = False, stereo_offset_exponent: float = 1.0) -> torch.Tensor:
    """input_images [B,C,H,W], depthmaps [B,H,W] -> [2B,C,H,W]: left views (the input unless shift_both) then right views."""
    if not torch.cuda.is_available():
        raise RuntimeError("comfystereo_amd needs an MI355X (PyTorch-ROCm `cuda` device); there is no CPU fallback")
    if depthmaps.dtype != torch.float32:
        # the reference normalises, applies pow and multiplies in the depth tensor's OWN dtype (stereo_utils.py:44-58); the
        # destination columns of a half / bfloat16 depth map round differently from a float32 one, and only float32 is pinned
        raise TypeError(f"stereo_shift_torch: depthmaps must be float32 (got {depthmaps.dtype}); parity with the reference is "
                        "pinned for float32 depth only")
    dev = input_images.device if input_images.is_cuda else torch.device("cuda", torch.cuda.current_device())
    out = engine.stereo_shift(input_images.to(dev, torch.float32), depthmaps.to(dev, torch.float32), scale_factor, shift_both,
                              stereo_offset_exponent)
    out = out.to(input_images.dtype)
    return out if input_images.is_cuda else out.to(input_images.device)


# float16 / bfloat16 q, k, v of BNAttention and of diffusion_utils' hook: False = upcast, float32 kernels, cast back; True = the half
# kernels (cs_stereo_attention_half; under autograd cs_attention_half_fwd_lse / cs_attention_half_bwd)
HALF_ATTENTION = False


def _need_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("comfystereo_amd needs an MI355X (PyTorch-ROCm `cuda` device); there is no CPU fallback")


def _attention(q, k, v, num_heads, scale, mode, chunks=1):
    """engine.stereo_attention on q, k, v as the reference holds them ([(c s b h), n, d]).  float16 / bfloat16 inputs are upcast
    to float32 and the result is cast back: the products, the softmax and the sums are float32 throughout, which is MORE
    accurate than the reference's arithmetic in the tensors' own half precision (its result differs by half-precision
    rounding errors; only float32, the Standard pipeline's dtype -- reference model_loader.py:63-65 -- is pinned).
    With HALF_ATTENTION set, float16 / bfloat16 q, k, v of one dtype go to the half kernel as they are (a head dimension that
    is no multiple of 8, which that kernel does not take, keeps the upcast)."""
    _need_gpu()
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise TypeError(f"BNAttention: {name} must be a floating-point tensor")
        if t.requires_grad:
            raise RuntimeError(f"BNAttention: {name} requires grad; the fused attention is forward only (run under torch.no_grad(), "
                               "as the reference's pipeline does, stereodiffusion_nodes.py:575)")
    if scale is None:
        raise ValueError("BNAttention needs the keyword argument scale")
    dev = q.device if q.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if HALF_ATTENTION and q.dtype in (torch.float16, torch.bfloat16) and k.dtype == q.dtype and v.dtype == q.dtype and q.shape[-1] % 8 == 0:
        qh, kh, vh = (t.detach().to(dev).contiguous() for t in (q, k, v))
        out = engine.stereo_attention(qh, kh, vh, num_heads, float(scale), mode, chunks)
        return out if q.is_cuda else out.to(q.device)
    q32, k32, v32 = (t.detach().to(dev, torch.float32).contiguous() for t in (q, k, v))
    out = engine.stereo_attention(q32, k32, v32, num_heads, float(scale), mode, chunks).to(q.dtype)
    return out if q.is_cuda else out.to(q.device)


class BNAttention:
    """The reference's attention editor (stereo_utils.py:91-188): from `start_step` on, every self-attention lets the right
    view's queries see the left view's keys ('uni') or both views see both ('bi').  Same constructor, attributes and call
    signatures; `sim` and `attn` are accepted for compatibility and ignored (they may be None): the fused kernel recomputes
    the scores tile by tile and never stores them."""

    def __init__(self, start_step: int = 4, total_steps: int = 50, direction: str = 'uni', use_cfg: bool = True):
        # the editor's whole state: four settings and two counters; register_attention_editor_diffusers fills in the layer count
        self.start_step, self.total_steps = start_step, total_steps
        self.direction, self.use_cfg = direction, use_cfg
        self.cur_step = self.cur_att_layer = 0
        self.num_att_layers = 0

    def attn_batch(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        """One CFG half in stereo mode (:119-133): q [(s b h), n, d] over the keys of both views, or -- k, v [(b h), n, d],
        the left view's half, as the reference's `forward` passes them for 'uni' -- over the left view's.  That second form
        costs a copy of k and v (the kernel addresses the left view inside a two-view tensor); `forward` here never takes it."""
        if k.shape[0] == q.shape[0]:
            return _attention(q, k, v, num_heads, kwargs.get("scale"), "bi")
        if 2 * k.shape[0] != q.shape[0]:
            raise ValueError(f"attn_batch: {q.shape[0]} query and {k.shape[0]} key batch entries")
        # the kernel addresses the left view inside a [(s b h)] tensor: hand it one whose view 0 is k, v (view 1 is not read)
        return _attention(q, torch.cat([k, k]), torch.cat([v, v]), num_heads, kwargs.get("scale"), "uni")

    def forward(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        if is_cross or (self.cur_step < self.start_step):
            return _attention(q, k, v, num_heads, kwargs.get("scale"), "self")   # (:137-140)
        if not self.use_cfg:
            return _attention(q, k, v, num_heads, kwargs.get("scale"), "bi")     # (:142-146) [left, right]
        # CFG: the batch is [uncond_left, uncond_right, cond_left, cond_right] (:148-176)
        if self.direction not in ('bi', 'uni'):
            raise ValueError(f"Unknown direction: {self.direction}")
        return _attention(q, k, v, num_heads, kwargs.get("scale"), self.direction, chunks=2)

    def __call__(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        out = self.forward(q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs)
        # one call per attention layer: the step is the number of complete passes over the registered layers (over 32 layers,
        # SD 1.x's count, for an editor nobody registered)
        self.cur_att_layer += 1
        self.cur_step = self.cur_att_layer // (self.num_att_layers if self.num_att_layers > 0 else 32)
        return out


_SAVED_FORWARD = "_comfystereo_saved_forward"


def _get_unet(model):
    """Where the reference looks for the UNet (:284-307), in its order: a ComfyUI wrapper's `comfy_model.model.diffusion_model`,
    a diffusers pipeline's `unet`, a raw ComfyUI model's `model.diffusion_model`; anything else is taken to be the UNet."""
    for path in (("comfy_model", "model", "diffusion_model"), ("unet",), ("model", "diffusion_model")):
        if path[0] == "comfy_model" and hasattr(model, "comfy_model"):
            return model.comfy_model.model.diffusion_model   # (no fall-through: the reference does not probe further here)
        node = model
        for name in path:
            node = getattr(node, name, None)
            if node is None:
                break
        else:
            return node
    return model


def _walk_attention(model, visit):
    """The reference's walk (:258-281): the UNet's children whose name says down / input, mid, up / output, and below them
    every module whose class name contains 'Attention' and that has children.  visit(module, place_in_unet); returns the count."""
    def walk(net, count, place_in_unet):
        for _name, subnet in net.named_children():
            if 'Attention' in net.__class__.__name__:
                visit(net, place_in_unet)
                return count + 1
            elif hasattr(net, 'children'):
                count = walk(subnet, count, place_in_unet)
        return count

    total = 0
    for net_name, net in _get_unet(model).named_children():
        if "down" in net_name or "input" in net_name:
            total += walk(net, 0, "down")
        elif "mid" in net_name:
            total += walk(net, 0, "mid")
        elif "up" in net_name or "output" in net_name:
            total += walk(net, 0, "up")
    return total


def register_attention_editor_diffusers(model, editor: BNAttention):
    """Install `editor` on every attention module of the model's UNet (reference :190-281: the same walk, the same names) and
    count the modules into editor.num_att_layers.  The installed forward computes q, k, v with the module's own linear layers
    and calls the editor with sim = attn = None: no score matrix is built.  The original forwards are saved on the modules;
    restore_attention puts them back.
    An attention mask other than None is refused with ValueError: Stable Diffusion's UNet never passes one, and the fused
    kernel has no mask input."""
    def install(net, place_in_unet):
        if not hasattr(net, _SAVED_FORWARD):
            # an instance attribute shadows the class's forward: remember whether there was one
            setattr(net, _SAVED_FORWARD, net.__dict__.get("forward"))
        scale = net.scale if hasattr(net, 'scale') else net.dim_head ** -0.5

        def forward(x, encoder_hidden_states=None, attention_mask=None, context=None, mask=None, value=None,
                    transformer_options=None, **kwargs):
            # diffusers' and ComfyUI's names for the same two things; the first of each pair wins, as in the reference
            context = encoder_hidden_states if encoder_hidden_states is not None else context
            mask = attention_mask if attention_mask is not None else mask
            if mask is not None:
                raise ValueError("the fused stereo attention takes no attention mask")
            is_cross = context is not None
            source = context if is_cross else x
            heads = net.heads

            def split(t):   # [b, n, heads * d] -> [(b heads), n, d]
                b, n, hd = t.shape
                return t.reshape(b, n, heads, hd // heads).permute(0, 2, 1, 3).reshape(b * heads, n, hd // heads)

            q, k = split(net.to_q(x)), split(net.to_k(source))
            v = split(net.to_v(source if value is None else value))
            out = editor(q, k, v, None, None, is_cross, place_in_unet, heads, scale=scale)
            project = net.to_out[0] if isinstance(net.to_out, nn.ModuleList) else net.to_out
            return project(out)

        net.forward = forward

    editor.num_att_layers = _walk_attention(model, install)


def restore_attention(model):
    """Put back the forwards register_attention_editor_diffusers replaced (reference :310-393 installs a plain attention
    forward instead; here the modules get their own forward back, which computes the same thing)."""
    def uninstall(net, place_in_unet):
        if hasattr(net, _SAVED_FORWARD):
            saved = getattr(net, _SAVED_FORWARD)
            delattr(net, _SAVED_FORWARD)
            if saved is None:
                net.__dict__.pop("forward", None)
            else:
                net.forward = saved

    _walk_attention(model, uninstall)
