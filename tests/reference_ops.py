"""The CPU specification the HIP kernels are held to: a conv layer's forward, input and weight gradient, the InstanceNorm / BatchNorm +
PReLU backward, the Boundary loss, the per-voxel terms and the gradient of the label losses.  torch only, in the precision of the arguments (float64: the reference; float32: the evaluation a
bound is measured from); nothing here touches the library.  tests/test_reference_ops.py checks this file against autograd."""
import torch
import torch.nn.functional as F


def rounded(t, dt):
    """``t`` rounded to the torch dtype ``dt`` (the storage type), as float32"""
    return t.detach().to(dt).float()


def softmax64(x):
    return torch.softmax(x.double(), dim=-1)


# ---- one conv layer ----------------------------------------------------------------------------------------------------------
# kind: "conv" (stride 1, "same" padding), "conv_s2" (stride 2, padding (k - 1) // 2), "convT" (3-tap transposed, stride 2, padding 1,
# output padding 1: doubles every extent).  The rank is ``dims`` where a module is built and that of the tensor elsewhere.
def conv_module(kind, cin, cout, k=3, dims=3):
    conv, convT = (torch.nn.Conv3d, torch.nn.ConvTranspose3d) if dims == 3 else (torch.nn.Conv2d, torch.nn.ConvTranspose2d)
    if kind == "convT":
        return convT(cin, cout, 3, 2, 1, output_padding=1)
    return conv(cin, cout, k, 2 if kind == "conv_s2" else 1, (k - 1) // 2)


def conv_fwd(kind, k, x, w, b):
    two_d = x.ndim == 4
    if kind == "convT":
        return (F.conv_transpose2d if two_d else F.conv_transpose3d)(x, w, b, stride=2, padding=1, output_padding=1)
    return (F.conv2d if two_d else F.conv3d)(x, w, b, stride=2 if kind == "conv_s2" else 1, padding=(k - 1) // 2)


def conv_dgrad(kind, k, gy, w, x_shape):
    """input gradient of the same layer: the transposed operator, no bias"""
    two_d = gy.ndim == 4
    if kind == "convT":
        return (F.conv2d if two_d else F.conv3d)(gy, w, None, stride=2, padding=1)
    s = 2 if kind == "conv_s2" else 1
    p = (k - 1) // 2
    op = tuple(x_shape[2 + i] - ((gy.shape[2 + i] - 1) * s - 2 * p + k) for i in range(gy.ndim - 2))
    return (F.conv_transpose2d if two_d else F.conv_transpose3d)(gy, w, None, stride=s, padding=p, output_padding=op)


def conv_out_shape(kind, k, spatial):
    """spatial extents of the layer's output for an input of extents ``spatial``"""
    if kind == "convT":
        return tuple(2 * v for v in spatial)
    s = 2 if kind == "conv_s2" else 1
    return tuple((v + 2 * ((k - 1) // 2) - k) // s + 1 for v in spatial)


def conv_wgrad(kind, k, x, dy, wshape, dtype):
    """autograd weight / bias gradient of the layer at (x, dy) in ``dtype``"""
    w = torch.zeros(wshape, dtype=dtype, requires_grad=True)
    b = torch.zeros(dy.shape[1], dtype=dtype, requires_grad=True)
    conv_fwd(kind, k, x.to(dtype), w, b).backward(dy.to(dtype))
    return w.grad.detach(), b.grad.detach()


# ---- InstanceNorm / BatchNorm + PReLU backward ----------------------------------------------------------------------------------
def norm_prelu_terms(g, y, mean, rstd, alpha, gamma=None, beta=None):
    """xhat = (y - mean) * rstd, dz (the gradient behind the PReLU, whose pre-activation is xhat, or gamma * xhat + beta with an
    affine norm) and the three terms the backward sums: (dz, dz * xhat, g * min(pre-activation, 0): the slope's gradient).
    mean, rstd, gamma, beta broadcast against y; alpha: a number or a tensor"""
    xh = (y - mean) * rstd
    pre = xh if gamma is None else gamma * xh + beta
    dz = g * torch.where(pre > 0, torch.ones_like(pre), torch.as_tensor(alpha, dtype=pre.dtype))
    return xh, dz, (dz, dz * xh, torch.where(pre > 0, torch.zeros_like(pre), g * pre))


def norm_prelu_dy(g, y, mean, rstd, alpha, gamma=None, beta=None, dims=(2, 3, 4)):
    """dL/dy of norm + PReLU; ``dims``: the axes one set of statistics spans ((2, 3, 4) per sample and channel; (0, 2) a batch of
    flattened samples)"""
    xh, dz, (t1, t2, _) = norm_prelu_terms(g, y, mean, rstd, alpha, gamma, beta)
    scale = rstd if gamma is None else gamma * rstd
    return scale * (dz - t1.mean(dims, keepdim=True) - xh * t2.mean(dims, keepdim=True))


# ---- Boundary loss ---------------------------------------------------------------------------------------------------------------
def boundary_weights64(ind, exclude_missing, B, K):
    """weight of T[b, c] in the scalar, float64: the plain mean, or models/losses.py:206-221 (non-Focal branch)"""
    if not exclude_missing:
        return torch.full((B, K), 1.0 / (B * K), dtype=torch.float64)
    ind = ind.double()
    w = 1.0 / ind.sum(dim=0)
    if torch.any(torch.isinf(w)):
        w = torch.ones_like(w)
    w = w / w.sum()
    return w[None, :] * ind / B


def boundary64(logits, sides):
    """sides: [(maps (B, C-1, *spatial), weights (B, C-1) float64)] -> (value, its magnitude sum, gradient, sum_j |g_j| p_j), float64:
    the scalar sum_s sum_bc W_s T(D_s), T[b, c] the mean over the sample of p[b, c + 1] D[b, c]"""
    x = logits.double().requires_grad_(True)
    p = torch.softmax(x, dim=1)
    sp = tuple(range(2, x.ndim))
    val = sum(((p[:, 1:] * D.double()).mean(dim=sp) * Wt).sum() for D, Wt in sides)
    mag = sum(((p[:, 1:] * D.double()).abs().mean(dim=sp) * Wt.abs()).sum() for D, Wt in sides)
    grad = torch.autograd.grad(val, x)[0]
    S = logits[0, 0].numel()
    gk = torch.zeros_like(p)
    for D, Wt in sides:
        gk[:, 1:] += Wt.reshape(Wt.shape + (1,) * len(sp)) * D.double() / S
    return val.item(), mag.item(), grad, (gk.abs() * p).sum(dim=1, keepdim=True).detach()


# ---- label losses: cross-entropy, soft Dice / focal sums, prediction, Dice counts ---------------------------------------------------
def first_max_index(v):
    """first index along the last axis at which ``v`` takes its maximum"""
    C = v.shape[-1]
    at_max = v == v.max(dim=-1, keepdim=True).values
    return torch.where(at_max, torch.arange(C), torch.full((), C, dtype=torch.int64)).min(dim=-1).values


def dice_count_table(pred, labels, C):
    """(..., S) predictions and labels -> (..., 3, C) int64: |pred == c & label == c|, |pred == c|, |label == c|; values >= C count nowhere"""
    cls = torch.arange(C)
    p, t = pred.long()[..., None] == cls, labels.long()[..., None] == cls
    return torch.stack([(p & t).sum(-2), p.sum(-2), t.sum(-2)], dim=-2)


def seg_loss_terms(x, labels, C, class_weight=None):
    """per voxel, in the precision of ``x`` (logits (..., S, >= C), labels (..., S) < C): ce = w (lse - x_t) and w (the class weight of
    the label, or 1); p = softmax, py = p * onehot, fo = (1 - p_t)^2 (-log p_t) at the label's class; pred = softmax THEN the first
    maximal index; cnt (..., 3, C) = the Dice counts of pred against the labels"""
    x = x[..., :C]
    lab = labels.long()
    oh = F.one_hot(lab, C).to(x.dtype)
    logp = torch.log_softmax(x, -1)
    p = torch.softmax(x, -1)
    logpt, pt = (logp * oh).sum(-1), (p * oh).sum(-1)
    w = torch.ones_like(logpt) if class_weight is None else class_weight.to(x.dtype)[lab]
    pred = first_max_index(p)
    return dict(ce=w * -logpt, w=w, p=p, py=p * oh, fo=((1 - pt) ** 2 * -logpt)[..., None] * oh, pred=pred,
                cnt=dice_count_table(pred, lab, C))


def seg_loss_records(terms, ce_only=False):
    """the terms of seg_loss_terms as one row per voxel in the order of a partial record: (ce, w, p[C], py[C], fo[C]); ``ce_only``:
    the cross-entropy-only pass, whose entries from 2 on are 0"""
    soft = torch.cat([terms["p"], terms["py"], terms["fo"]], -1)
    return torch.cat([terms["ce"][..., None], terms["w"][..., None], torch.zeros_like(soft) if ce_only else soft], -1)


def seg_loss_grad(x, labels, C, coef, cw):
    """d L / d x in the precision of ``x`` (logits (B, S, C)) by autograd, L the scalar one coefficient row per sample defines:
    coef (B, 1 + 3 C) = (s, a[C], b[C], f[C]), cw (C,) class weights:
    L = sum_voxels  s w_t (-log p_t)  +  sum_c (a_c [c = t] + b_c) p_c  +  f_t (1 - p_t)^2 (-log p_t)"""
    xr = x[..., :C].detach().clone().requires_grad_(True)
    dt = xr.dtype
    p = torch.softmax(xr, -1)
    oh = F.one_hot(labels.long(), C).to(dt)
    logp = torch.log_softmax(xr, -1)
    pt, logpt = (p * oh).sum(-1), (logp * oh).sum(-1)
    cf = coef.to(dt)
    a, b_, f = cf[:, None, 1:1 + C], cf[:, None, 1 + C:1 + 2 * C], cf[:, None, 1 + 2 * C:]
    w = cw.to(dt)[labels.long()]
    L = (cf[:, None, 0] * w * -logpt).sum() + ((a * oh + b_) * p).sum() + ((f * oh).sum(-1) * -(1 - pt) ** 2 * logpt).sum()
    return torch.autograd.grad(L, xr)[0]
