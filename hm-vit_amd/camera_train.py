"""Training path of the camera branch (VERDICT r2 missing #1): what ``ResnetEncoder`` (``opencood/models/backbones/resnet_ms.py:8-89``,
torchvision BasicBlock / Bottleneck trunks), ``CrossViewModule`` / ``CrossViewAttention`` / ``CrossAttention``
(``sub_modules/cvt_modules.py:95-331``) and the up-sampling ``NaiveDecoder`` (``naive_decoder.py:63-92``) compute under
``nn.Module.train()`` with autograd - the reference trains the camera backbone unless ``--fix_camera_backbone``
(``tools/train_camera.py:109-120``).  BatchNorm works on batch statistics and updates its running buffers; every parameter of the
branch receives its gradient.

Every multiply-accumulate over pixels / tokens runs in libhmvit behind ``torch.autograd.Function``s:

  * 3 x 3 convolutions (stride 1 / 2), BatchNorm on batch statistics (+ ReLU), 1 x 1 convolutions   hm-vit_amd/tail_train.py
  * Linear (f32 operands, products on split-f16 operands; dW = dY^T X as ``hmvit_gemm_tn``)           ``LinearFn``
  * LayerNorm forward / backward, erf GELU forward / backward                                           ``LayerNormFn`` / ``GeluFn``
  * the joint-softmax cross attention over all cameras' keys, forward with the row log-sum-exp and a two-kernel backward
    (``hmvit_cross_attention_train`` / ``_backward``, csrc/cvt.hip)                                     ``CrossAttnFn``

Glue left to torch tensor plumbing (no matrix products): layout changes, im2col of the 3-channel 7 x 7 stem (its products
are a ``LinearFn`` over the unfolded patches), max pooling and nearest up-sampling (value routing), residual adds / ReLU, and the
ray / camera / BEV positional embeddings (1 x 1 "convolutions" over 2 or 4 geometric channels: a handful of broadcast
multiply-adds, L2 normalisation).
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from . import tail_train as TT


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _pad_cols(t, mult):
    k = t.shape[-1]
    kp = (k + mult - 1) // mult * mult
    return t if kp == k else F.pad(t, (0, kp - k))


class LinearFn(torch.autograd.Function):
    """y (M, N) = x (M, K) w^T (+ b); f32, products on split-f16 operands (HMVIT_PREC_SPLIT).  K and N are zero-padded to the
    kernels' granules (64 for a contraction axis, 4 for ``hmvit_gemm_tn``'s N / K) where they are not multiples already."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        M, K = x.shape
        w2 = weight.detach().reshape(weight.shape[0], -1)
        N = w2.shape[0]
        xp, wp = _pad_cols(x, 64).contiguous(), _pad_cols(w2, 64).contiguous()
        y = torch.empty(M, N, device=x.device, dtype=torch.float32)
        b = bias.detach().float().contiguous() if bias is not None else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib.hmvit_linear(xp.data_ptr(), wp.data_ptr(), b.data_ptr() if b is not None else None, None, y.data_ptr(),
                                             M, N, xp.shape[1], 0, 1, _lib.PREC_SPLIT, _stream(x.device)), "linear")
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy, un = _lib.grad_pow2(dy)                      # split-f16 products: run on dy 2^k, results times 2^-k (exact)
        M, K = x.shape
        w2 = weight.detach().reshape(weight.shape[0], -1)
        N = w2.shape[0]
        dev = x.device
        dx = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                dyp = _pad_cols(dy, 64).contiguous()                                  # contraction over N
                wt = torch.zeros(K, dyp.shape[1], device=dev, dtype=torch.float32)
                wt[:, :N] = w2.t()
                dx = torch.empty(M, K, device=dev, dtype=torch.float32)
                _lib.check(_lib.lib.hmvit_linear(dyp.data_ptr(), wt.data_ptr(), None, None, dx.data_ptr(), M, K, dyp.shape[1], 0, 1,
                                                 _lib.PREC_SPLIT, _stream(dev)), "linear(dgrad)")
            dy4, x4 = _pad_cols(dy, 4).contiguous(), _pad_cols(x, 4).contiguous()
            Np, Kp = dy4.shape[1], x4.shape[1]
            dw = torch.zeros(Np, Kp, device=dev, dtype=torch.float32)
            db = torch.zeros(Np, device=dev, dtype=torch.float32)
            _lib.check(_lib.lib.hmvit_gemm_tn(dy4.data_ptr(), x4.data_ptr(), dw.data_ptr(), db.data_ptr(), M, Np, Kp, Np, Kp, _stream(dev)),
                       "gemm_tn")
        return (dx * un if dx is not None else None, dw[:N, :K].reshape(weight.shape).contiguous() * un,
                db[:N].contiguous() * un if ctx.has_bias else None)


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm(C) over the rows of x (M, C), C in {64, 128, 256}."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        if abs(eps - 1e-5) > 1e-12:
            raise NotImplementedError("LayerNorm kernel: eps = 1e-5")
        x = x.contiguous()
        M, C = x.shape
        g, b = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib.hmvit_layernorm(x.data_ptr(), y.data_ptr(), _lib.i32_array([0]), g.data_ptr(), b.data_ptr(), 1, M, C,
                                                _lib.PREC_F32, _stream(x.device)), "layernorm")
        ctx.save_for_backward(x, g)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g = ctx.saved_tensors
        dy = dy.contiguous()
        M, C = x.shape
        dx = torch.empty_like(x)
        dg = torch.zeros(C, device=x.device, dtype=torch.float32)
        db = torch.zeros(C, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib.hmvit_layernorm_backward(x.data_ptr(), dy.data_ptr(), g.data_ptr(), dx.data_ptr(), dg.data_ptr(),
                                                         db.data_ptr(), M, C, _stream(x.device)), "layernorm_backward")
        return dx, dg, db, None


class GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib.hmvit_gelu(x.data_ptr(), y.data_ptr(), x.numel(), _stream(x.device)), "gelu")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib.hmvit_gelu_backward(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), _stream(x.device)), "gelu_backward")
        return dx


class CrossAttnFn(torch.autograd.Function):
    """q (b, n, Q, HD), k (b, n, K, HD), v (b, n K, HD) -> a (b, Q, HD): softmax over the keys of ALL n cameras
    (cvt_modules.py:141-149), exact f32."""

    @staticmethod
    def forward(ctx, q, k, v, heads, dim_head):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        b, n, Q, HD = q.shape
        K = k.shape[2]
        a = torch.empty(b, Q, HD, device=q.device, dtype=torch.float32)
        lse = torch.empty(b, heads, Q, device=q.device, dtype=torch.float32)
        with torch.cuda.device(q.device):
            _lib.check(_lib.lib.hmvit_cross_attention_train(q.data_ptr(), k.data_ptr(), v.data_ptr(), a.data_ptr(), lse.data_ptr(), b, n, Q, K,
                                                            heads, dim_head, _stream(q.device)), "cross_attention_train")
        ctx.save_for_backward(q, k, v, a, lse)
        ctx.dims = (heads, dim_head)
        return a

    @staticmethod
    def backward(ctx, da):
        q, k, v, a, lse = ctx.saved_tensors
        heads, dim_head = ctx.dims
        da = da.contiguous()
        b, n, Q, HD = q.shape
        K = k.shape[2]
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        with torch.cuda.device(q.device):
            _lib.check(_lib.lib.hmvit_cross_attention_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), a.data_ptr(), lse.data_ptr(),
                                                               da.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), b, n, Q, K, heads,
                                                               dim_head, _stream(q.device)), "cross_attention_backward")
        return dq, dk, dv, None, None


class AttnBiasFn(torch.autograd.Function):
    """q (b, Q, HD), k / v (b, K, HD), bias (heads, Q, K) -> (b, Q, HD): softmax(q k^T / sqrt(32) + bias) v per head, exact f32 -
    the self-attention that closes FAXModule (fax_modules.py:136-180) on libhmvit (``hmvit_attention_bias_train`` / ``_backward``)."""

    @staticmethod
    def forward(ctx, q, k, v, bias, heads, dim_head):
        q, k, v, bias = q.contiguous(), k.contiguous(), v.contiguous(), bias.contiguous().float()
        b, Q, HD = q.shape
        K = k.shape[1]
        a = torch.empty(b, Q, HD, device=q.device, dtype=torch.float32)
        lse = torch.empty(b, heads, Q, device=q.device, dtype=torch.float32)
        with torch.cuda.device(q.device):
            _lib.check(_lib.lib.hmvit_attention_bias_train(q.data_ptr(), k.data_ptr(), v.data_ptr(), bias.data_ptr(), a.data_ptr(), lse.data_ptr(),
                                                           b, Q, K, heads, dim_head, _stream(q.device)), "attention_bias_train")
        ctx.save_for_backward(q, k, v, bias, a, lse)
        ctx.dims = (heads, dim_head)
        return a

    @staticmethod
    def backward(ctx, da):
        q, k, v, bias, a, lse = ctx.saved_tensors
        heads, dim_head = ctx.dims
        da = da.contiguous()
        b, Q, HD = q.shape
        K = k.shape[1]
        dq, dk, dv, dbias = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(bias)
        with torch.cuda.device(q.device):
            _lib.check(_lib.lib.hmvit_attention_bias_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), bias.data_ptr(), a.data_ptr(), lse.data_ptr(),
                                                              da.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dbias.data_ptr(), b, Q, K,
                                                              heads, dim_head, _stream(q.device)), "attention_bias_backward")
        return dq, dk, dv, dbias, None, None


class MaxPoolFn(torch.autograd.Function):
    """nn.MaxPool2d on an f32 NHWC map: ``hmvit_maxpool2d`` forward, ``hmvit_maxpool2d_backward`` (the gradient of a window goes to its
    first maximum in row-major order) - the ResNet stem's 3 x 3 / 2 pooling under autograd (resnet_ms.py:71)."""

    @staticmethod
    def forward(ctx, x, ksize, stride, pad):
        x = x.contiguous()
        n, h, w, c = x.shape
        ho, wo = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
        y = torch.empty(n, ho, wo, c, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib.hmvit_maxpool2d(x.data_ptr(), y.data_ptr(), n, h, w, c, ksize, stride, pad, _lib.PREC_F32, _stream(x.device)),
                       "maxpool2d")
        ctx.save_for_backward(x)
        ctx.dims = (ksize, stride, pad)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        ksize, stride, pad = ctx.dims
        n, h, w, c = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib.hmvit_maxpool2d_backward(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, h, w, c, ksize, stride, pad,
                                                         _stream(x.device)), "maxpool2d_backward")
        return dx, None, None, None


# ---------------------------------------------------------------------------------------------------------------------
# layers
# ---------------------------------------------------------------------------------------------------------------------
def linear(x2d, lin):
    return LinearFn.apply(x2d, lin.weight, lin.bias)


def layer_norm(x2d, ln):
    return LayerNormFn.apply(x2d, ln.weight, ln.bias, ln.eps)


def conv1x1(t, conv, stride: int = 1):
    """NHWC 1 x 1 convolution (optionally strided: a sub-sampling of the map) as a Linear over the pixels."""
    if stride != 1:
        t = t[:, ::stride, ::stride]
    n, H, W, C = t.shape
    return LinearFn.apply(t.reshape(-1, C), conv.weight, conv.bias).reshape(n, H, W, -1)


def conv3x3(t, conv):
    return TT.Conv3x3.apply(t, conv.weight, conv.bias, conv.stride[0])


def basic_block(blk, t):
    """torchvision BasicBlock: conv3x3 (stride) - BN - ReLU - conv3x3 - BN, + identity / (1x1 strided conv - BN), ReLU."""
    idt = t if blk.downsample is None else TT.bn_relu_module(conv1x1(t, blk.downsample[0], blk.downsample[0].stride[0]), blk.downsample[1],
                                                              relu=False)
    y = TT.bn_relu_module(conv3x3(t, blk.conv1), blk.bn1)
    y = TT.bn_relu_module(conv3x3(y, blk.conv2), blk.bn2, relu=False)
    return torch.relu(y + idt)


def bottleneck_block(blk, t):
    """torchvision Bottleneck (v1.5: the stride sits on the 3 x 3): 1x1 - BN - ReLU - 3x3 - BN - ReLU - 1x1 - BN, + identity, ReLU."""
    ds = getattr(blk, "downsample", None)
    idt = t if ds is None else TT.bn_relu_module(conv1x1(t, ds[0], ds[0].stride[0]), ds[1], relu=False)
    y = TT.bn_relu_module(conv1x1(t, blk.conv1), blk.bn1)
    y = TT.bn_relu_module(conv3x3(y, blk.conv2), blk.bn2)
    y = TT.bn_relu_module(conv1x1(y, blk.conv3), blk.bn3, relu=False)
    return torch.relu(y + idt)


def resnet_encoder_forward(enc, input_images):
    """``ResnetEncoder.forward`` in training mode: (b, l, m, h, w, 3) images -> list of (b, l, m, C, h', w') pyramid levels."""
    e = enc.encoder
    b, l, m, h, w, c = input_images.shape
    img = input_images.reshape(b * l * m, h, w, c).float()
    # 7 x 7 / stride 2 stem on 3 channels: im2col (data movement) + a Linear over the 147-tap patches
    conv = e.conv1
    k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    cols = F.unfold(img.permute(0, 3, 1, 2), k, padding=p, stride=s)                 # (n, 3 k k, L), channel-major taps like the weight
    Ho, Wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    x = LinearFn.apply(cols.transpose(1, 2).reshape(-1, cols.shape[1]), conv.weight, conv.bias).reshape(b * l * m, Ho, Wo, -1)
    x = TT.bn_relu_module(x, e.bn1)
    x = MaxPoolFn.apply(x, 3, 2, 1)                                                      # value routing on libhmvit
    outs = []
    for li in range(4):
        for blk in getattr(e, f"layer{li + 1}"):
            x = bottleneck_block(blk, x) if hasattr(blk, "conv3") else basic_block(blk, x)
        f = x.permute(0, 3, 1, 2)
        outs.append(f.reshape(b, l, m, *f.shape[1:]))
    return [outs[i] for i in enc.idx_pick] if isinstance(enc.idx_pick, list) else outs[enc.idx_pick]


def _small_matmul(a, b):
    """(..., r, c) x (..., c, m) for c <= 4 (camera geometry): c broadcast multiply-adds."""
    return sum(a[..., :, j:j + 1] * b[..., j:j + 1, :] for j in range(a.shape[-1]))


def _small_conv(x, conv):
    """1 x 1 convolution over 2 or 4 geometric channels, (N, c, h, w) -> (N, dim, h, w): c broadcast multiply-adds."""
    w = conv.weight[:, :, 0, 0]
    y = sum(w[None, :, ci, None, None] * x[:, ci:ci + 1] for ci in range(x.shape[1]))
    return y if conv.bias is None else y + conv.bias[None, :, None, None]


def cross_attention_forward(ca, q, k, v, skip):
    """``CrossAttention.forward`` (cvt_modules.py:119-165) on token-major tensors: q (b, n, Q, dim), k (b, n, K, dim),
    v (b, n K, dim), skip (b, Q, dim) or None -> (b, Q, dim)."""
    b, n, Q, dim = q.shape
    qp = linear(layer_norm(q.reshape(-1, dim), ca.to_q[0]), ca.to_q[1]).reshape(b, n, Q, -1)
    kp = linear(layer_norm(k.reshape(-1, dim), ca.to_k[0]), ca.to_k[1]).reshape(b, n, k.shape[2], -1)
    vp = linear(layer_norm(v.reshape(-1, dim), ca.to_v[0]), ca.to_v[1]).reshape(b, v.shape[1], -1)
    a = CrossAttnFn.apply(qp, kp, vp, ca.heads, ca.dim_head)
    z = linear(a.reshape(b * Q, -1), ca.proj)
    if skip is not None:
        z = z + skip.reshape(-1, dim)
    z = layer_norm(z, ca.prenorm)
    z = z + linear(GeluFn.apply(linear(z, ca.mlp[0])), ca.mlp[2])
    z = layer_norm(z, ca.postnorm)
    return z.reshape(b, Q, dim)


def cross_view_attention_forward(cva, x, bev, feature, I_inv, E_inv):
    """``CrossViewAttention.forward`` (cvt_modules.py:213-280) in training mode: x (b, dim, H, W), feature (b, n, C, h, w)."""
    from .cvt import generate_grid
    b, n, C, h, w = feature.shape
    _, dim, H, W = x.shape
    dev = x.device
    pixel = generate_grid(h, w)[None].to(dev)                       # 1 1 3 h w
    pixel = pixel * torch.tensor([cva.image_width, cva.image_height, 1.0], device=dev).view(1, 1, 3, 1, 1)
    c = E_inv[..., -1:].reshape(b * n, 4, 1, 1)                     # camera centres
    c_embed = _small_conv(c, cva.cam_embed)                          # (b n) dim 1 1
    cam = _small_matmul(I_inv.reshape(b, n, 3, 3), pixel.reshape(1, 1, 3, h * w))   # pixel rays (geometry, no parameters)
    cam = F.pad(cam, (0, 0, 0, 1), value=1.0)
    d = _small_matmul(E_inv.reshape(b, n, 4, 4), cam).reshape(b * n, 4, h, w)
    img_embed = _small_conv(d, cva.img_embed) - c_embed
    img_embed = img_embed / (img_embed.norm(dim=1, keepdim=True) + 1e-7)
    w_embed = _small_conv(bev.grid[:2][None].to(dev), cva.bev_embed)  # 1 dim H W
    bev_embed = w_embed - c_embed
    bev_embed = bev_embed / (bev_embed.norm(dim=1, keepdim=True) + 1e-7)
    query = bev_embed.reshape(b, n, dim, H, W) + x[:, None]

    feat = feature.reshape(b * n, C, h, w).permute(0, 2, 3, 1).contiguous()       # NHWC
    key = img_embed.permute(0, 2, 3, 1)                                # key before value, as cvt_modules.py:133-139 evaluates them
    if cva.feature_proj is not None:
        key = key + conv1x1(TT.bn_relu_module(feat, cva.feature_proj[0]), cva.feature_proj[2])
    val = conv1x1(TT.bn_relu_module(feat, cva.feature_linear[0]), cva.feature_linear[2])
    q_tok = query.permute(0, 1, 3, 4, 2).reshape(b, n, H * W, dim)
    k_tok = key.reshape(b, n, h * w, dim)
    v_tok = val.reshape(b, n * h * w, dim)
    skip = x.permute(0, 2, 3, 1).reshape(b, H * W, dim) if cva.skip else None
    z = cross_attention_forward(cva.cross_attend, q_tok, k_tok, v_tok, skip)
    return z.reshape(b, H, W, dim).permute(0, 3, 1, 2)


def cross_view_module_forward(cvm, batch):
    """``CrossViewModule.forward`` (cvt_modules.py:314-331) in training mode -> (b, l, dim, H, W)."""
    b, l, n = batch["inputs"].shape[:3]
    I_inv = torch.linalg.inv_ex(batch["intrinsic"].reshape(b * l, n, 3, 3).float())[0]   # (inv_ex: no host read of the status)
    E_inv = batch["extrinsic"].reshape(b * l, n, 4, 4).float()
    x = cvm.bev_embedding.get_prior()[None].expand(b * l, -1, -1, -1)
    for cross_view, feature, layer in zip(cvm.cross_views, batch["features"], cvm.layers):
        feature = feature.reshape(b * l, n, *feature.shape[3:])
        x = cross_view_attention_forward(cross_view, x, cvm.bev_embedding, feature, I_inv, E_inv)
        if len(layer):
            t = x.permute(0, 2, 3, 1).contiguous()
            for blk in layer:
                t = bottleneck_block(blk, t)
            x = t.permute(0, 3, 1, 2)
    return x.reshape(b, l, *x.shape[1:])


def naive_decoder_forward(dec, x_nchw, use_upsample=True, nhwc=False):
    """``NaiveDecoder.forward`` (naive_decoder.py:63-92) on (N, C, H, W): per layer conv - BN - ReLU, nearest x2, conv - BN - ReLU.
    ``nhwc``: return the map as (N, H, W, C) (for 1x1 heads that read it in that layout)."""
    t = x_nchw.permute(0, 2, 3, 1).contiguous()
    layers = dec.decoder
    for i in range(0, len(layers), 6):
        t = TT.bn_relu_module(conv3x3(t, layers[i]), layers[i + 1])
        if use_upsample:
            t = t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        t = TT.bn_relu_module(conv3x3(t, layers[i + 3]), layers[i + 4])
    return t if nhwc else t.permute(0, 3, 1, 2).contiguous()


def cvt_camera_encoder_forward(enc, batch_camera):
    """``CvtCameraEncoder.forward`` in training mode: images -> ResNet pyramid -> cross-view lift -> decoder -> (N, 256, Hb, Wb)."""
    cam = batch_camera["camera"]
    feats = resnet_encoder_forward(enc.encoder, cam[None])
    x = cross_view_module_forward(enc.cvm, {"inputs": cam[None], "intrinsic": batch_camera["intrinsic"][None],
                                            "extrinsic": batch_camera["extrinsic"][None], "features": feats})[0]
    return naive_decoder_forward(enc.decoder, x, use_upsample=True)
