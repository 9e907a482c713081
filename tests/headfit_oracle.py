"""fp64 restatement of the head fit for the tests: the regression head's L1 loss, its gradients and AdamW.  torch on the CPU,
no autograd: every formula is written out, so that the tests of this build's kernels do not lean on the code they test.

Head: pre = X Wa^T + ba, A = leaky_relu(pre, 0.01), z = A Wb^T + bb, sigma = sigmoid(z) (act 0) | tanh(z) (act 1), s = sigma^p, and
s[b Np + i gw + j, P py + px] is pixel (b, P i + py, P j + px) of the score map (the jigsaw of utils/misc/image.py:8-21).
loss = inv_count * sum |s - gt|;  g = sign(s - gt) ds/dz (sign(0) = 0, as torch.abs's backward has it), WITHOUT the factor inv_count;
dbb = inv_count * sum_m g, dWb = inv_count * g^T A, dA = g Wb, dpre = dA * (A > 0 ? 1 : 0.01), dba = inv_count * sum_m dpre, dWa = inv_count * dpre^T X.
`rnd` (a function fp64 -> fp64, or None) rounds g and dpre where the kernels round them to the 16-bit operand type.

AdamW is torch.optim.AdamW's documented single-tensor algorithm (amsgrad off, maximize off):
    theta <- theta - lr * lambda * theta;  m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;
    m_hat = m / (1 - beta1^t);  v_hat = v / (1 - beta2^t);  theta <- theta - lr * m_hat / (sqrt(v_hat) + eps),   t = 1, 2, ..."""
import torch

F64 = torch.float64
LEAKY = 0.01


def to_rows(img, gh, gw, P):
    """(B, gh P, gw P) image -> (B gh gw, P P) rows in the head's column order (the inverse jigsaw)"""
    B = img.shape[0]
    return img.reshape(B, gh, P, gw, P).permute(0, 1, 3, 2, 4).reshape(B * gh * gw, P * P)


def to_image(rows, B, gh, gw, P):
    """(B gh gw, P P) rows -> (B, gh P, gw P): jigsaw_to_image"""
    return rows.reshape(B, gh, gw, P, P).permute(0, 1, 3, 2, 4).reshape(B, gh * P, gw * P)


def leaky(x):
    return torch.where(x > 0, x, LEAKY * x)


def activation(z, act, p):
    """-> (sigma, s, ds/dz, |d2s/dz2|)"""
    if act == 0:
        sg = torch.sigmoid(z)
        s = sg ** p
        d1 = p * sg ** (p - 1) * sg * (1 - sg)            # p sigma^p (1 - sigma)
        d2 = d1 * (p * (1 - sg) - sg)                     # d/dz of p sigma^p (1 - sigma)
    else:
        sg = torch.tanh(z)
        s = sg ** p
        d1 = (p * sg ** (p - 1) if p != 1 else torch.ones_like(sg)) * (1 - sg * sg)
        d2 = -2 * sg * (1 - sg * sg) if p == 1 else torch.full_like(sg, float("nan"))
    return sg, s, d1, d2.abs()


def scores(A, Wb, bb, act, p):
    """s (M, P P) and z from the hidden rows"""
    z = A.to(F64) @ Wb.to(F64).T + bb.to(F64)
    return activation(z, act, p)[1], z


def grad_z(A, Wb, bb, gt_rows, act, p):
    """-> (g (M, P P) unrounded, sum |s - gt|, s, z)"""
    s, z = scores(A, Wb, bb, act, p)
    d = s - gt_rows.to(F64)
    g = torch.sign(d) * activation(z, act, p)[2]
    return g, d.abs().sum(), s, z


def backward(X, A, Wb, bb, gt_rows, act, p, inv_count, rnd=None):
    """-> dict(dWa, dba, dWb, dbb, loss, g, dpre): g and dpre as `rnd` left them"""
    rnd = rnd or (lambda t: t)
    X, A, Wb = X.to(F64), A.to(F64), Wb.to(F64)
    g, lsum, _, _ = grad_z(A, Wb, bb, gt_rows, act, p)
    g = rnd(g)
    dpre = rnd((g @ Wb) * torch.where(A > 0, torch.ones_like(A), torch.full_like(A, LEAKY)))  # (fp64 tensors: python scalars would make the mask fp32)
    return {"dWa": inv_count * (dpre.T @ X), "dba": inv_count * dpre.sum(0), "dWb": inv_count * (g.T @ A), "dbb": inv_count * g.sum(0),
            "loss": inv_count * lsum, "g": g, "dpre": dpre}


def adamw_step(p, m, v, g, step, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """one step, out of place, in the dtype of its inputs (fp64 in the tests) -> (p, m, v)"""
    b1, b2 = betas
    p = p - lr * weight_decay * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    m_hat = m / (1 - b1 ** step)
    v_hat = v / (1 - b2 ** step)
    return p - lr * m_hat / (v_hat.sqrt() + eps), m, v


def step_lr(lr0, step_size, gamma, n):
    """StepLR: the rate in force after n scheduler steps"""
    return lr0 * gamma ** (n // step_size)


def fit(X, params, gt_rows, act, p, steps, lr=5e-4, step_size=None, gamma=1.0, **adam):
    """`steps` AdamW steps of the head on one fixed batch in fp64 (X fixed: the encoder and decoder are frozen) -> (losses before each step,
    final params); params = [Wa, ba, Wb, bb]; StepLR(step_size, gamma) stepped once per optimiser step when step_size is given"""
    X = X.to(F64)
    params = [t.to(F64).clone() for t in params]
    m = [torch.zeros_like(t) for t in params]
    v = [torch.zeros_like(t) for t in params]
    inv = 1.0 / gt_rows.numel()
    losses = []
    for t in range(1, steps + 1):
        Wa, ba, Wb, bb = params
        A = leaky(X @ Wa.T + ba)
        r = backward(X, A, Wb, bb, gt_rows, act, p, inv)
        losses.append(float(r["loss"]))
        rate = step_lr(lr, step_size, gamma, t - 1) if step_size else lr
        for k, key in enumerate(("dWa", "dba", "dWb", "dbb")):
            params[k], m[k], v[k] = adamw_step(params[k], m[k], v[k], r[key], t, lr=rate, **adam)
    return losses, params
