"""Plain references of the normalisation, loss-head and optimiser kernels of include/emloco_predictor.h.

Every function restates one operation of the header from its documented contract and the reference project's formulas, never from a
kernel: closed forms in torch, evaluated in the dtype given (float64 by default).  tests/test_kernel_refs_cpu.py pins each of them
against torch autograd / torch.optim / torch.nn.functional of the textbook expression; tests/test_gpu_elementwise_matrix.py compares
the device kernels with them.  Calling one with dtype=torch.float32 evaluates the same operation with stock float32 torch on the CPU:
its distance to the float64 result is the "float32-reference error" the device bars are derived from.

No kernel, no library, no GPU is needed to import or run this module.
"""
import math

import torch

F64 = torch.float64
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
LV_HIDDEN_JOINTS = (4, 8, 9, 10, 11)        # value_pose_net.py:141-144: joints zeroed in the MLP input
LV_SIZES = (4900, 49, 1176, 24, 24, 1)      # dparams layout of emloco_locoval_bwd: dw1 | db1 | dw2 | db2 | dw3 | db3


def _c(t, dtype):
    return None if t is None else torch.as_tensor(t).detach().to("cpu").to(dtype)


def bf16_round(x):
    """round-to-nearest-even to bf16, back as float64"""
    return torch.as_tensor(x).float().to(torch.bfloat16).double()


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm (post-norm encoder layer: y = LayerNorm(x + res) gamma + beta, biased variance)

def layernorm_fwd(x, res, gamma, beta, eps, dtype=F64):
    """-> y, mean [rows], rstd [rows], xr = x + res"""
    x, res, gamma, beta = _c(x, dtype), _c(res, dtype), _c(gamma, dtype), _c(beta, dtype)
    xr = x if res is None else x + res
    mean = xr.mean(dim=-1)
    c = xr - mean[:, None]
    rstd = 1.0 / torch.sqrt((c * c).mean(dim=-1) + eps)
    return c * rstd[:, None] * gamma + beta, mean, rstd, xr


def layernorm_bwd(xr, gamma, mean, rstd, dy, dy2=None, dtype=F64):
    """-> dxr, dgamma, dbeta for the incoming gradient dy (+ dy2); mean / rstd as the forward saved them"""
    xr, gamma, mean, rstd, dy, dy2 = (_c(t, dtype) for t in (xr, gamma, mean, rstd, dy, dy2))
    if dy2 is not None:
        dy = dy + dy2
    xh = (xr - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dxr = rstd[:, None] * (g - g.mean(dim=-1, keepdim=True) - xh * (g * xh).mean(dim=-1, keepdim=True))
    return dxr, (dy * xh).sum(dim=0), dy.sum(dim=0)


def layernorm_bwd_terms(xr, gamma, mean, rstd, dy, dy2=None):
    """sum |terms| of the dgamma / dbeta reductions (the scale of a fixed-order fp32 sum's error)"""
    xr, gamma, mean, rstd, dy, dy2 = (_c(t, F64) for t in (xr, gamma, mean, rstd, dy, dy2))
    if dy2 is not None:
        dy = dy + dy2
    xh = (xr - mean[:, None]) * rstd[:, None]
    return (dy * xh).abs().sum(dim=0), dy.abs().sum(dim=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax over attention scores with an additive per-key bias

def softmax_fwd(S, scale, key_bias=None, rows_per_seq=1, dtype=F64):
    """S [rows][cols]; key_bias [n_seq][cols] or None; a row whose keys are all -inf gives zeros"""
    S, key_bias = _c(S, dtype), _c(key_bias, dtype)
    z = S * scale
    if key_bias is not None:
        z = z + key_bias.repeat_interleave(rows_per_seq, dim=0)
    dead = torch.isneginf(z).all(dim=-1, keepdim=True)
    p = torch.softmax(torch.where(dead, torch.zeros_like(z), z), dim=-1)
    return torch.where(dead, torch.zeros_like(p), p)


def softmax_bwd(P, dP, scale, dtype=F64):
    P, dP = _c(P, dtype), _c(dP, dtype)
    return scale * P * (dP - (dP * P).sum(dim=-1, keepdim=True))


# ---------------------------------------------------------------------------------------------------------------------------------
# epilogue backward, column sums

def act_bwd(dy, y, relu, keep, p, dtype=F64):
    """dz = dy [relu: y > 0] [dropout: keep / (1 - p)]; with ReLU a positive forward output already means "active and kept" """
    dy, y = _c(dy, dtype), _c(y, dtype)
    v = dy
    if relu:
        v = torch.where(y > 0, v, torch.zeros_like(v))
    if p > 0:
        inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
        v = v * inv.to(dtype)                     # the documented scale is the float32 value 1 / (1 - p)
        if not relu:
            v = v * _c(keep, dtype)
    return v


def colsum(X, dtype=F64):
    return _c(X, dtype).sum(dim=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# policy-input normaliser, AMP style reward, running moments

def obs_normalize(x, mean, var, eps, clip, dtype=F64):
    x, mean, var = _c(x, dtype), _c(mean, dtype), _c(var, dtype)
    return torch.clamp((x - mean) / torch.sqrt(var + eps), -clip, clip)


def disc_reward(logits, scale, dtype=F64):
    """-log(max(1 - sigmoid(logit), 1e-4)) * scale"""
    x = _c(logits, dtype)
    prob = 1.0 / (1.0 + torch.exp(-x))
    return -torch.log(torch.clamp_min(1.0 - prob, 0.0001)) * scale


def disc_one_minus_sigmoid(logits):
    return 1.0 - 1.0 / (1.0 + torch.exp(-_c(logits, F64)))


def rms_update(x, mean, var, count, first_col=0):
    """RunningMeanStd.forward in training mode: the batch's mean and UNBIASED variance merged with the parallel-variance rule;
    columns below first_col keep their moments.  float64 throughout.  -> mean, var, count"""
    x, mean, var = _c(x, F64), _c(mean, F64).clone(), _c(var, F64).clone()
    n = x.shape[0]
    bm = x.mean(dim=0)
    bv = ((x - bm) ** 2).sum(dim=0) / (n - 1.0) if n > 1 else torch.full_like(bm, float("nan"))
    d = bm - mean
    tot = count + n
    new_mean = mean + d * n / tot
    new_var = (var * count + bv * n + d * d * count * n / tot) / tot
    mean[first_col:] = new_mean[first_col:]
    var[first_col:] = new_var[first_col:]
    return mean, var, tot


# ---------------------------------------------------------------------------------------------------------------------------------
# chained feed-forward block on bf16 operands (the hidden layer and dz1 are stored as bf16 once)

def ffn_fwd(x, w1, b1, w2, b2, keep_h=None, keep_o=None, p=0.0, rounded=True):
    """x [M][128], w1 [F][128], w2 [128][F]; keep_h [M][F], keep_o [M][128] 0/1 or None.
    -> hidden (as stored: bf16-rounded), active-and-kept mask [M][F] (bool), out [M][128], the pre-activation z1 (for branch distances)"""
    r = bf16_round if rounded else (lambda t: _c(t, F64))
    x, w1, w2, b1, b2 = r(x), r(w1), r(w2), _c(b1, F64), _c(b2, F64)
    inv = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32)))
    z1 = x @ w1.T + b1
    h = z1.clamp_min(0.0)
    active = z1 > 0
    if p > 0:
        h = h * _c(keep_h, F64) * inv
        active = active & (_c(keep_h, F64) > 0)
    hidden = bf16_round(h) if rounded else h
    out = hidden @ w2.T + b2
    if p > 0:
        out = out * _c(keep_o, F64) * inv
    return hidden, active, out, z1


def ffn_bwd_input(dz2, w1, w2, active, p=0.0, rounded=True):
    """dz1 = (dz2 w2) o active / (1 - p) (stored bf16), dx = dz1 w1"""
    r = bf16_round if rounded else (lambda t: _c(t, F64))
    inv = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32)))
    dz1 = (r(dz2) @ r(w2)) * _c(active, F64) * inv
    dz1 = bf16_round(dz1) if rounded else dz1
    return dz1, dz1 @ r(w1)


# ---------------------------------------------------------------------------------------------------------------------------------
# LocoVal MLP with yaw normalisation (value_pose_net.py:36-159)

def locoval_input(traj, pose, vel):
    """traj [B][13][>=2], pose [B][24][3], vel [B][2] -> x100 [B][100], angle [B] (differentiable in traj)"""
    x1, y1 = traj[:, 1, 0], traj[:, 1, 1]
    x1 = torch.where(x1.abs() < 1e-10, torch.full_like(x1, 1e-10), x1)         # epsilon guard on x (:79-83): a constant, no gradient
    ang = torch.atan2(y1, x1)
    c, s = torch.cos(ang)[:, None], torch.sin(ang)[:, None]

    def rot(px, py):
        return px * c + py * s, -px * s + py * c
    tx, ty = rot(traj[:, :, 0], traj[:, :, 1])
    px, py = rot(pose[:, :, 0], pose[:, :, 1])
    vx, vy = rot(vel[:, 0:1], vel[:, 1:2])
    live = torch.ones(24, dtype=traj.dtype)
    live[list(LV_HIDDEN_JOINTS)] = 0.0
    p3 = torch.stack([px, py, pose[:, :, 2]], dim=-1) * live[None, :, None]
    x100 = torch.cat([torch.stack([tx, ty], dim=-1).reshape(-1, 26), p3.reshape(-1, 72), vx, vy], dim=1)
    return x100, ang


def locoval_fwd(traj, pose, vel, params, dtype=F64):
    """params = (w1 [49][100], b1, w2 [24][49], b2, w3 [24], b3 [1]) -> value [B], x100, h1, h2, angle"""
    traj, pose, vel = _c(traj, dtype), _c(pose, dtype), _c(vel, dtype)
    w1, b1, w2, b2, w3, b3 = (_c(t, dtype) for t in params)
    x100, ang = locoval_input(traj, pose, vel)
    h1 = torch.relu(x100 @ w1.reshape(49, 100).T + b1)
    h2 = torch.relu(h1 @ w2.reshape(24, 49).T + b2)
    value = torch.sigmoid(h2 @ w3.reshape(24) + b3.reshape(()))
    return value, x100, h1, h2, ang


def locoval_bwd(traj, pose, vel, params, dvalue, dtype=F64):
    """-> dparams [6174] (summed over the batch), d traj [B][13][stride] (zero beyond x, y).  Gradients by autograd of the restated
    forward."""
    traj = _c(traj, dtype).clone().requires_grad_(True)
    ps = [_c(t, dtype).clone().requires_grad_(True) for t in params]
    value = locoval_fwd_graph(traj, _c(pose, dtype), _c(vel, dtype), ps)
    dv = _c(dvalue, dtype)
    grads = torch.autograd.grad((value * dv).sum(), [traj] + ps)
    return torch.cat([g.reshape(-1) for g in grads[1:]]), grads[0]


def locoval_fwd_graph(traj, pose, vel, ps):
    w1, b1, w2, b2, w3, b3 = ps
    x100, _ = locoval_input(traj, pose, vel)
    h1 = torch.relu(x100 @ w1.reshape(49, 100).T + b1)
    h2 = torch.relu(h1 @ w2.reshape(24, 49).T + b2)
    return torch.sigmoid(h2 @ w3.reshape(24) + b3.reshape(()))


def locoval_input_mag(traj, pose, vel):
    """the error scale of every element of x100: a rotation by an angle that carries a rounding error d moves a point p by |p| d, so a
    rotated coordinate is judged against |p_x| + |p_y| of its point, not against its own size (the rotated y of waypoint 1 is ~0 by
    construction: the yaw normalisation turns that waypoint onto the x axis)"""
    traj, pose, vel = _c(traj, F64), _c(pose, F64), _c(vel, F64)
    t = traj[:, :, 0].abs() + traj[:, :, 1].abs()
    p = pose[:, :, 0].abs() + pose[:, :, 1].abs()
    v = (vel[:, 0].abs() + vel[:, 1].abs())[:, None]
    live = torch.ones(24, dtype=F64)
    live[list(LV_HIDDEN_JOINTS)] = 0.0
    p3 = torch.stack([p, p, pose[:, :, 2].abs()], dim=-1) * live[None, :, None]
    return torch.cat([torch.stack([t, t], dim=-1).reshape(-1, 26), p3.reshape(-1, 72), v, v], dim=1)


def locoval_bwd_terms(traj, pose, vel, params, dvalue):
    """sum over the batch of |per-row parameter gradient| [6174]: the error scale of the fixed-order batch sum.  For dw1 the row's term
    is |d1_j| x the MAGNITUDE of x100_k (locoval_input_mag), not |x100_k|."""
    B = traj.shape[0]
    tot = torch.zeros(sum(LV_SIZES), dtype=F64)
    xmag = locoval_input_mag(traj, pose, vel)
    for i in range(B):
        dp, _ = locoval_bwd(traj[i:i + 1], pose[i:i + 1], vel[i:i + 1], params, dvalue[i:i + 1])
        dp = dp.abs()
        dp[:4900] = (dp[4900:4949, None] * xmag[i][None, :]).reshape(-1)
        tot += dp
    return tot


# ---------------------------------------------------------------------------------------------------------------------------------
# LocoVal fit: gradient of the sum-reduced MSE over the rows with a target, AdamW, clip + Adam

def fit_grad(value, target, weight, dtype=F64):
    """-> dvalue [n], loss sum, row count, slot [n] (rank among the valid rows, -1 elsewhere).  A weight-0 row contributes nothing,
    whatever its value holds (NaN included)."""
    value, target, weight = _c(value, dtype), _c(target, dtype), _c(weight, dtype)
    live = weight != 0
    d = torch.where(live, value - target, torch.zeros_like(value))
    slot = torch.where(live, torch.cumsum(live.long(), 0) - 1, torch.full_like(live.long(), -1)).to(torch.int32)
    return 2.0 * weight * d, (weight * d * d).sum(), int(live.sum()), slot


def adamw_step(p, g, m, v, step, lr, b1, b2, eps, wd, dtype=F64):
    """torch.optim.AdamW, step = the count AFTER this step.  -> p, m, v"""
    p, g, m, v = (_c(t, dtype) for t in (p, g, m, v))
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps)), m, v


def clip_coef(g, max_norm):
    """clip_grad_norm_: -> total norm, coefficient min(1, max_norm / (norm + 1e-6)) (float64 tensors; NaN stays NaN)"""
    norm = _c(g, F64).pow(2).sum().sqrt()
    c = max_norm / (norm + 1e-6)
    return norm, torch.where(c < 1.0, c, torch.where(torch.isnan(c), c, torch.ones_like(c)))


def adam_clip_step(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm, dtype=F64):
    """clip_grad_norm_(max_norm) + torch.optim.Adam (L2 weight decay).  -> p, g (left clipped), m, v, norm, coefficient"""
    p, g, m, v = (_c(t, dtype) for t in (p, g, m, v))
    norm = coef = None
    if max_norm > 0:
        norm = g.pow(2).sum().sqrt()
        c = max_norm / (norm + 1e-6)
        coef = torch.where(c < 1.0, c, torch.where(torch.isnan(c), c, torch.ones_like(c)))
        g = g * coef
    ge = g + wd * p if wd != 0 else g
    m = m + (1.0 - b1) * (ge - m)
    v = v * b2 + (1.0 - b2) * ge * ge
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    return p - (lr / bc1) * (m / (v.sqrt() / bc2s + eps)), g, m, v, norm, coef


# ---------------------------------------------------------------------------------------------------------------------------------
# PPO heads

def neglogp(actions, mu, logstd):
    return 0.5 * (((actions - mu) / torch.exp(logstd)) ** 2).sum(dim=-1) + HALF_LOG_2PI * actions.shape[-1] + logstd.sum(dim=-1)


def actor_rows(mu, logstd, actions, old_neglogp, adv, old_mu, old_sigma, e_clip):
    """per-row [surrogate, entropy, bound loss, clipped 0/1, KL(new || old)] and the ratio"""
    nlp = neglogp(actions, mu, logstd)
    ratio = torch.exp(old_neglogp - nlp)
    sur = torch.maximum(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - e_clip, 1.0 + e_clip))
    ent = (0.5 + HALF_LOG_2PI + logstd).sum(dim=-1)
    bound = (torch.clamp_max(mu + 1.0, 0.0) ** 2 + torch.clamp_min(mu - 1.0, 0.0) ** 2).sum(dim=-1)
    clipped = ((ratio - 1.0).abs() > e_clip).to(mu.dtype)
    if old_mu is None:
        kl = torch.zeros_like(sur)
    else:
        s = torch.exp(logstd)
        kl = (torch.log(old_sigma / s + 1e-5) + (s ** 2 + (old_mu - mu) ** 2) / (2.0 * (old_sigma ** 2 + 1e-5)) - 0.5).sum(dim=-1)
    return torch.stack([sur, ent, bound, clipped, kl], dim=1), ratio


def actor_head_fwd(mu, logstd, actions, old_neglogp, adv, old_mu, old_sigma, e_clip, dtype=F64):
    """-> out5 (means over the rows), per-row values [B][5], ratio [B]"""
    a = [_c(t, dtype) for t in (mu, logstd, actions, old_neglogp, adv, old_mu, old_sigma)]
    rows, ratio = actor_rows(*a, e_clip)
    return rows.mean(dim=0), rows, ratio


def actor_head_bwd(mu, logstd, actions, old_neglogp, adv, e_clip, grad3, dtype=F64):
    """d(g0 mean surrogate + g1 mean entropy + g2 mean bound) / d(mu, logstd); torch's maximum hands a tie half to each side and clamp
    passes the gradient on its closed interval"""
    mu, logstd, actions, old_neglogp, adv, g = (_c(t, dtype) for t in (mu, logstd, actions, old_neglogp, adv, grad3))
    B = mu.shape[0]
    s = torch.exp(logstd)
    t = (actions - mu) / s
    ratio = torch.exp(old_neglogp - neglogp(actions, mu, logstd))
    lo, hi = 1.0 - e_clip, 1.0 + e_clip
    s1, s2 = -adv * ratio, -adv * torch.clamp(ratio, lo, hi)
    w1 = torch.where(s1 > s2, 1.0, torch.where(s1 == s2, 0.5, 0.0)).to(dtype)
    inr = ((ratio >= lo) & (ratio <= hi)).to(dtype)
    c_nlp = (g[0] / B * adv * ratio * (w1 + (1.0 - w1) * inr))[:, None]
    dmu = c_nlp * (-t / s) + g[2] / B * 2.0 * (torch.clamp_max(mu + 1.0, 0.0) + torch.clamp_min(mu - 1.0, 0.0))
    dlogstd = c_nlp * (1.0 - t * t) + g[1] / B
    return dmu, dlogstd


def critic_rows(v, v_old, ret, e_clip, clip_value):
    if clip_value:
        vc = v_old + torch.clamp(v - v_old, -e_clip, e_clip)
        return torch.maximum((v - ret) ** 2, (vc - ret) ** 2)
    return (ret - v) ** 2


def critic_head_fwd(v, v_old, ret, e_clip, clip_value, dtype=F64):
    rows = critic_rows(_c(v, dtype), _c(v_old, dtype), _c(ret, dtype), e_clip, clip_value)
    return rows.mean(), rows


def critic_head_bwd(v, v_old, ret, e_clip, clip_value, grad1, dtype=F64):
    v, v_old, ret, g = _c(v, dtype), _c(v_old, dtype), _c(ret, dtype), _c(grad1, dtype)
    d1 = v - ret
    grad = 2.0 * d1
    if clip_value:
        dlt = v - v_old
        d2 = v_old + torch.clamp(dlt, -e_clip, e_clip) - ret
        l1, l2 = d1 * d1, d2 * d2
        w1 = torch.where(l1 > l2, 1.0, torch.where(l1 == l2, 0.5, 0.0)).to(dtype)
        inr = ((dlt >= -e_clip) & (dlt <= e_clip)).to(dtype)
        grad = w1 * 2.0 * d1 + (1.0 - w1) * 2.0 * d2 * inr
    return g.reshape(-1)[0] * grad / v.shape[0]


def bce_logits(x, target):
    """BCEWithLogits per element: max(x, 0) - x t + log(1 + exp(-|x|))"""
    return torch.clamp_min(x, 0.0) - x * target + torch.log1p(torch.exp(-x.abs()))


def disc_head_fwd(agent, demo, dtype=F64):
    """-> out4 = [mean bce(agent, 0), fraction agent < 0, mean bce(demo, 1), fraction demo > 0], per-row bce of both groups"""
    a, d = _c(agent, dtype), _c(demo, dtype)
    ra, rd = bce_logits(a, 0.0), bce_logits(d, 1.0)
    return torch.stack([ra.mean(), (a < 0).to(dtype).mean(), rd.mean(), (d > 0).to(dtype).mean()]), ra, rd


def disc_head_bwd(agent, demo, grad2, dtype=F64):
    a, d, g = _c(agent, dtype), _c(demo, dtype), _c(grad2, dtype)
    return g[0] * torch.sigmoid(a) / a.shape[0], g[1] * (torch.sigmoid(d) - 1.0) / d.shape[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# error measures and branch distances

def err_max(got, ref):
    """max |got - ref| over the tensor's own scale max |ref| (normalised outputs)"""
    got, ref = _c(got, F64), _c(ref, F64)
    assert torch.isfinite(got).all(), "non-finite output (an element not written, or a bad value)"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def err_terms(got, ref, terms):
    """max |got - ref| / sum |terms| (sums and dot products)"""
    got, ref, terms = _c(got, F64), _c(ref, F64), _c(terms, F64)
    assert torch.isfinite(got).all(), "non-finite output (an element not written, or a bad value)"
    return ((got - ref).abs() / terms.clamp_min(1e-300)).max().item()


def near_share(dist, scale, rel=1e-5):
    """share of the elements whose float64 distance to a branch point is below rel x the operand scale"""
    dist = _c(dist, F64).abs()
    return (dist < rel * scale).double().mean().item()


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs of the random cases with a branch in them (shared by the CPU test, which counts their near-branch elements, and the
# device matrix, which runs them)

def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def case_actor(B, A, seed):
    """mu / logstd / actions / old statistics of a PPO minibatch: ratios spread over both sides of the clip range, some mu beyond +-1"""
    g = _gen(seed)
    mu = torch.randn(B, A, generator=g) * 0.7
    logstd = torch.randn(B, A, generator=g) * 0.1 - 1.0
    actions = mu + torch.exp(logstd) * torch.randn(B, A, generator=g)
    old_mu = mu + 0.05 * torch.randn(B, A, generator=g)
    old_sigma = torch.exp(logstd + 0.05 * torch.randn(B, A, generator=g))
    nlp = neglogp(actions.double(), mu.double(), logstd.double())
    old_neglogp = (nlp + 0.3 * torch.randn(B, generator=g).double()).float()
    adv = torch.randn(B, generator=g)
    return dict(mu=mu, logstd=logstd, actions=actions, old_neglogp=old_neglogp, adv=adv, old_mu=old_mu, old_sigma=old_sigma)


def actor_branch_distances(c, e_clip):
    """float64 distances of a case to its branch points: ratio to the clip edges (relative to 1), mu to +-1"""
    d = {k: v.double() for k, v in c.items()}
    ratio = torch.exp(d["old_neglogp"] - neglogp(d["actions"], d["mu"], d["logstd"]))
    edge = torch.minimum((ratio - (1.0 - e_clip)).abs(), (ratio - (1.0 + e_clip)).abs())
    bound = torch.minimum((d["mu"] - 1.0).abs(), (d["mu"] + 1.0).abs())
    return edge, bound


def case_critic(B, seed):
    g = _gen(seed)
    v_old = torch.randn(B, generator=g)
    v = v_old + 0.3 * torch.randn(B, generator=g)
    ret = v_old + 0.5 * torch.randn(B, generator=g)
    return dict(v=v, v_old=v_old, ret=ret)


def critic_branch_distances(c, e_clip):
    """distance of v - v_old to +-e, and of the two losses to each other (where they are not the same expression)"""
    v, v_old, ret = c["v"].double(), c["v_old"].double(), c["ret"].double()
    dlt = v - v_old
    edge = torch.minimum((dlt - e_clip).abs(), (dlt + e_clip).abs())
    l1 = (v - ret) ** 2
    l2 = (v_old + torch.clamp(dlt, -e_clip, e_clip) - ret) ** 2
    tie = torch.where(dlt.abs() <= e_clip, torch.full_like(l1, float("inf")), (l1 - l2).abs())
    return edge, tie


def case_locoval(B, stride, seed):
    g = _gen(seed)
    traj = torch.zeros(B, 13, stride)
    traj[:, :, :2] = torch.cumsum(torch.randn(B, 13, 2, generator=g) * 0.3 + torch.tensor([0.5, 0.1]), dim=1)
    traj[:, 0] = 0
    if stride > 2:
        traj[:, :, 2:] = torch.randn(B, 13, stride - 2, generator=g) * 50.0        # must not enter anything
    pose = torch.randn(B, 24, 3, generator=g) * 0.3
    vel = torch.randn(B, 2, generator=g)
    params = [torch.randn(49, 100, generator=g) * 0.15, torch.randn(49, generator=g) * 0.1, torch.randn(24, 49, generator=g) * 0.2,
              torch.randn(24, generator=g) * 0.1, torch.randn(24, generator=g) * 0.3, torch.randn(1, generator=g) * 0.1]
    dvalue = torch.randn(B, generator=g)
    return dict(traj=traj, pose=pose, vel=vel, params=params, dvalue=dvalue)


def locoval_branch_distances(c):
    """pre-activations of the two ReLU layers (distance to 0) in float64"""
    traj, pose, vel = c["traj"].double(), c["pose"].double(), c["vel"].double()
    w1, b1, w2, b2 = (t.double() for t in c["params"][:4])
    x100, _ = locoval_input(traj, pose, vel)
    z1 = x100 @ w1.T + b1
    z2 = torch.relu(z1) @ w2.T + b2
    return z1, z2


def case_ffn(M, F, seed):
    g = _gen(seed)
    return dict(x=torch.randn(M, 128, generator=g), w1=torch.randn(F, 128, generator=g) * 0.09, b1=torch.randn(F, generator=g) * 0.1,
                w2=torch.randn(128, F, generator=g) * (1.0 / math.sqrt(F)), b2=torch.randn(128, generator=g) * 0.1,
                dz2=torch.randn(M, 128, generator=g), res=torch.randn(M, 128, generator=g),
                gamma=1.0 + 0.1 * torch.randn(128, generator=g), beta=0.1 * torch.randn(128, generator=g))


def case_obs(rows, cols, seed):
    g = _gen(seed)
    mean = torch.randn(cols, generator=g)
    var = torch.rand(cols, generator=g) * 2.0 + 0.05
    x = mean + torch.sqrt(var) * torch.randn(rows, cols, generator=g) * 2.5      # ~4.5 % beyond the clamp at 5
    return dict(x=x, mean=mean, var=var)


# ---------------------------------------------------------------------------------------------------------------------------------
# device-matrix bookkeeping shared by the conformance matrices

MARGIN = 8.0                            # device bar = MARGIN x the float32 reference's own error


class Table:
    """collects (float32-reference error, device error) per output of a family; asserts device <= MARGIN x max float32 error"""

    def __init__(self, family, executor="device"):
        self.family, self.rows, self.executor = family, [], executor

    def add(self, case, name, dev_err, f32_err):
        self.rows.append((case, name, dev_err, f32_err))

    def check(self):
        names = sorted({r[1] for r in self.rows})
        bad = []
        print()
        for n in names:
            f32 = max(r[3] for r in self.rows if r[1] == n)
            dev = max(r[2] for r in self.rows if r[1] == n)
            bar = MARGIN * f32
            print(f"  [{self.family}] {n:<12} float32 reference {f32:.3e}   bar {bar:.3e}   {self.executor} {dev:.3e}")
            bad += [(r[0], n, r[2], bar) for r in self.rows if r[1] == n and not r[2] <= bar]
        assert not bad, (f"{len(bad)} of {len(self.rows)} figures above {MARGIN} x the float32 reference's error", bad[:10])


# ---------------------------------------------------------------------------------------------------------------------------------
# the rollout's task kernels (include/emloco_task.h): quaternions are xyzw, every formula restated from the definitions the header
# cites (the reference's torch_utils helpers and observation builders), in the dtype given

F32 = torch.float32
LEFT_TO_RIGHT = (0, 5, 6, 7, 8, 1, 2, 3, 4, 9, 10, 11, 12, 13, 19, 20, 21, 22, 23, 14, 15, 16, 17, 18)
KEY_BODIES = (7, 3, 22, 17)
CONTACT_BODIES = (7, 3, 8, 4)
HEAD_BODY = 13
DOF_SUBSET = tuple(3 * j + k for j in range(23) if j not in (3, 7, 17, 22) for k in range(3))      # every joint but toes and hands


def quat_rotate(q, v):
    """my_quat_rotate: v (2 w^2 - 1) + 2 w (q_v x v) + 2 q_v (q_v . v)"""
    qv, w = q[..., :3], q[..., 3:4]
    qv, v = torch.broadcast_tensors(qv, v)
    return v * (2.0 * w * w - 1.0) + torch.cross(qv, v, dim=-1) * w * 2.0 + qv * (qv * v).sum(-1, keepdim=True) * 2.0


def quat_mul(a, b):
    """Hamilton product"""
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    return torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], dim=-1)


def _axis(q, k):
    e = torch.zeros(3, dtype=q.dtype)
    e[k] = 1.0
    return e


def calc_heading(q):
    """the angle about z of the rotated x axis"""
    r = quat_rotate(q, _axis(q, 0))
    return torch.atan2(r[..., 1], r[..., 0])


def quat_about_z(angle):
    z = torch.zeros_like(angle)
    return torch.stack([z, z, torch.sin(angle / 2.0), torch.cos(angle / 2.0)], dim=-1)


def heading_inv(q):
    return quat_about_z(-calc_heading(q))


def quat_to_tan_norm(q):
    return torch.cat([quat_rotate(q, _axis(q, 0)), quat_rotate(q, _axis(q, 2))], dim=-1)


def exp_map_to_quat(e):
    """rotation vector -> quaternion: the angle wrapped to (-pi, pi], an angle of at most 1e-5 is the identity"""
    angle = e.norm(dim=-1, keepdim=True)
    axis = e / angle
    angle = torch.atan2(torch.sin(angle), torch.cos(angle))
    small = ~(angle.abs() > 1e-5)
    angle = torch.where(small, torch.zeros_like(angle), angle)
    axis = torch.where(small, _axis(e, 2).expand_as(axis), axis)
    q = torch.cat([axis * torch.sin(angle / 2.0), torch.cos(angle / 2.0)], dim=-1)
    return q / q.norm(dim=-1, keepdim=True)


def pd_targets(actions, offset, scale, zero_mask, dtype=F64):
    """offset + scale a, exactly 0 where the mask is set"""
    a, o, s = _c(actions, dtype), _c(offset, dtype), _c(scale, dtype)
    m = torch.as_tensor(zero_mask).to("cpu") != 0
    return torch.where(m, torch.zeros_like(a), o + s * a)


def pd_targets_mag(actions, offset, scale):
    a, o, s = _c(actions, F64), _c(offset, F64), _c(scale, F64)
    return o.abs() + (s * a).abs()


def amp_row(root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_pos, betas, dof_subset=DOF_SUBSET, dtype=F64):
    """[n][35 + 3 n_sub] (206 for the shipped 57-entry subset): root rotation as tangent | normal in the heading frame (6), local root
    velocity and angular velocity (6), the subset's joints as tangent | normal (6 each), the subset's dof velocities, the key bodies
    relative to the root in the heading frame (12), betas[:11]"""
    rp, rr, rv, ra, dp, dv, kp, bt = (_c(t, dtype) for t in (root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_pos, betas))
    sub = torch.as_tensor(dof_subset).long()
    n = rp.shape[0]
    hinv = heading_inv(rr)
    joints = quat_to_tan_norm(exp_map_to_quat(dp[:, sub].reshape(n, -1, 3))).reshape(n, -1)
    keys = quat_rotate(hinv[:, None, :], kp.reshape(n, 4, 3) - rp[:, None, :]).reshape(n, 12)
    return torch.cat([quat_to_tan_norm(quat_mul(hinv, rr)), quat_rotate(hinv, rv), quat_rotate(hinv, ra), joints, dv[:, sub], keys, bt[:, :11]], dim=1)


def amp_blocks(n_sub=57):
    nj = n_sub // 3
    a = 12 + 6 * nj
    return (("rotation", 0, 6), ("velocity", 6, 12), ("dof_pos", 12, a), ("dof_vel", a, a + n_sub), ("key_pos", a + n_sub, a + n_sub + 12))


def self_obs(body_pos, body_rot, body_vel, body_ang_vel, betas, dtype=F64):
    """368 values: bodies 1..23 relative to the root in the heading frame (69), every body's rotation as tangent | normal (144), linear
    (72) and angular (72) velocities in the heading frame, betas[:11]"""
    p, r, v, a, bt = (_c(t, dtype) for t in (body_pos, body_rot, body_vel, body_ang_vel, betas))
    E = p.shape[0]
    hinv = heading_inv(r[:, 0])[:, None, :]
    local = quat_rotate(hinv, p - p[:, :1])[:, 1:]
    rot = quat_to_tan_norm(quat_mul(hinv.expand(E, 24, 4), r))
    return torch.cat([local.reshape(E, 69), rot.reshape(E, 144), quat_rotate(hinv, v).reshape(E, 72), quat_rotate(hinv, a).reshape(E, 72),
                      bt[:, :11]], dim=1)


def mirror_bodies(body_pos, body_rot, body_vel, body_ang_vel, left_to_right=LEFT_TO_RIGHT):
    """the left-right mirrored state: y of positions and velocities, x and z of rotations and angular velocities change sign, and
    the bodies trade places through left_to_right"""
    p, r, v, a = (torch.as_tensor(t).clone() for t in (body_pos, body_rot, body_vel, body_ang_vel))
    l2r = torch.as_tensor(left_to_right).long()
    p[..., 1] *= -1
    v[..., 1] *= -1
    r[..., 0] *= -1
    r[..., 2] *= -1
    a[..., 0] *= -1
    a[..., 2] *= -1
    return p[:, l2r], r[:, l2r], v[:, l2r], a[:, l2r]


def flip_self_obs(body_pos, body_rot, body_vel, body_ang_vel, betas, left_to_right=LEFT_TO_RIGHT, dtype=F64):
    return self_obs(*mirror_bodies(body_pos, body_rot, body_vel, body_ang_vel, left_to_right), betas, dtype=dtype)


def traj_calc_pos(verts, t, traj_dur, dtype=F64):
    """the polyline verts [E][V][3] at time t [E] or [E][k]: phase = clip(t / traj_dur, 0, 1), linear between the two vertices"""
    verts, t = _c(verts, dtype), _c(t, dtype)
    V = verts.shape[1]
    seg = torch.clamp(t / traj_dur, 0.0, 1.0) * (V - 1)
    i0, i1 = torch.floor(seg).long(), torch.ceil(seg).long()
    lerp = (seg - i0.to(dtype))[..., None]
    idx = lambda i: torch.gather(verts, 1, i.reshape(verts.shape[0], -1, 1).expand(-1, -1, 3)).reshape(*t.shape, 3)
    return (1.0 - lerp) * idx(i0) + lerp * idx(i1)


def traj_sample_times(progress, dt, sample_dt, n=15, dtype=F64):
    """progress dt + k sample_dt with dt and sample_dt as the float32 numbers the launch carries"""
    dt32, sdt32 = torch.tensor(dt, dtype=F32).to(dtype), torch.tensor(sample_dt, dtype=F32).to(dtype)
    return torch.as_tensor(progress).to(dtype)[:, None] * dt32 + torch.arange(n).to(dtype)[None, :] * sdt32


def location_obs(root, samples, dtype=F64):
    """root [E][>=7] (position, rotation), samples [E][k][3] -> [E][2 k]: x, y of sample - root in the heading frame"""
    root, samples = _c(root, dtype), _c(samples, dtype)
    hinv = heading_inv(root[:, 3:7])[:, None, :]
    return quat_rotate(hinv, samples - root[:, None, :3])[..., :2].reshape(root.shape[0], -1)


def reward(root_pos, target, dof_force, dof_vel, power_coef, dtype=F64):
    """-> rew, loc = exp(-2 |target - root|_xy^2), power = -coef sum |force x velocity|, and sum |terms| of the power sum"""
    rp, tg, f, v = (_c(t, dtype) for t in (root_pos, target, dof_force, dof_vel))
    coef = torch.tensor(power_coef, dtype=F32).to(dtype)
    d = tg[:, :2] - rp[:, :2]
    loc = torch.exp(-2.0 * (d * d).sum(-1))
    terms = (f * v).abs().sum(-1)
    power = -coef * terms
    return loc + power, loc, power, coef * terms


def reset_flags(progress, contact_force, contact_body_mask, root_pos, target, fail_dist, max_episode_length, dtype=F64):
    """-> reset, terminate (int64) and the distances of every env to the four thresholds [E][4]: |sum of the unmasked bodies' contact
    forces| - 50, |target - root|_xy^2 - fail_dist^2, progress - 1, progress - (max_episode_length - 1)"""
    cf, rp, tg = (_c(t, dtype) for t in (contact_force, root_pos, target))
    prog = torch.as_tensor(progress).to("cpu").to(dtype)
    live = (torch.as_tensor(contact_body_mask).to("cpu") == 0).to(dtype)
    s = (cf * live[None, :, None]).sum(dim=1)
    mag = torch.sqrt((s * s).sum(-1))
    d = tg[:, :2] - rp[:, :2]
    d2 = (d * d).sum(-1)
    dist = torch.stack([mag - 50.0, d2 - fail_dist * fail_dist, prog - 1.0, prog - (max_episode_length - 1.0)], dim=1)
    term = ((dist[:, 0] > 0) & (dist[:, 2] > 0)) | (dist[:, 1] > 0)
    reset = torch.where(dist[:, 3] >= 0, torch.ones_like(term), term)
    return reset.long(), term.long(), dist


def reset_near(dist, fail_dist, rel=1e-5):
    """envs within rel (relative) of a threshold of reset_flags: judged against the fp32 oracle only (progress is an integer: never near)"""
    return (dist[:, 0].abs() < rel * 50.0) | (dist[:, 1].abs() < rel * fail_dist * fail_dist)


def task_branch_distances(c):
    """float64 distances (with their scales) of a case_task state to every clamp / branch of the observations and flags:
    the +-3 clip of the height observations is measured where the heights exist (height_clip_distance); here: the 1e-5 and pi
    thresholds of the joints' rotation vectors, the clip of the trajectory phase, and the flags' thresholds"""
    dp = c["dof_state"][:, :, 0].double().reshape(-1, 23, 3).norm(dim=-1)
    t = traj_sample_times(c["progress"], c["dt"], c["sample_dt"]) / c["traj_dur"]
    _, _, dist = reset_flags(c["progress"], c["contact_force"], c["contact_body_mask"], c["rb_state"][:, 0, :3],
                             traj_calc_pos(c["traj_verts"], traj_sample_times(c["progress"], c["dt"], c["sample_dt"], 1), c["traj_dur"])[:, 0],
                             c["fail_dist"], c["max_episode_length"])
    return {"joint angle 1e-5": (dp - 1e-5, 1.0), "joint angle pi": (dp - math.pi, math.pi), "phase clip": (t - 1.0, 1.0),
            "contact 50 N": (dist[:, 0], 50.0), "fail distance": (dist[:, 1], c["fail_dist"] ** 2)}


def height_clip_distance(center_mean, heights):
    """|mean(centre) - h| - 3 of the height observations clip(mean(centre) - h, -3, 3) x 5"""
    return (_c(center_mean, F64)[:, None] - _c(heights, F64)).abs() - 3.0


def case_task(E, seed, max_episode_length=168.0):
    """A physically plausible but hard rollout state of E envs: roots 40-120 m from the origin (body - root and target - root cancel),
    headings over the full circle (some within 1e-3 of 0 and of +-pi), bodies pitched past vertical, progress over [0, max_len]
    (0, 1, 2, max_len - 2, max_len - 1 among them), contact-force sums from 0 to 200 N, targets on both sides of the fail distance."""
    g = _gen(seed)
    rnd = lambda *s: torch.rand(*s, generator=g)
    nrm = lambda *s: torch.randn(*s, generator=g)
    ang = (rnd(E) * 2.0 - 1.0) * math.pi
    special = torch.tensor([0.0, 5e-4, -5e-4, math.pi - 5e-4, -math.pi + 5e-4, math.pi - 1e-6, -math.pi + 1e-6])
    k = torch.arange(E)
    pick = (k % 5 == 1) | (E <= 7)
    ang = torch.where(pick, special[k % 7], ang)
    rad = 40.0 + 80.0 * rnd(E)
    phi = (rnd(E) * 2.0 - 1.0) * math.pi
    if E > 3:                                           # some envs in the negative quadrants, off the map's low sides
        phi[::4] = phi[::4].abs() * 0.5                 # ... and a quarter of them over the map
    root_pos = torch.stack([rad * torch.cos(phi), rad * torch.sin(phi), 0.85 + 0.2 * rnd(E)], dim=1)

    def quat(axis, a):
        axis = axis / axis.norm(dim=-1, keepdim=True)
        return torch.cat([axis * torch.sin(a / 2.0)[..., None], torch.cos(a / 2.0)[..., None]], dim=-1)

    yaw = quat(torch.tensor([0.0, 0.0, 1.0]).expand(E, 3), ang).double()
    pitch_a = torch.where((k % 3 == 0) & ~pick, 1.2 + 1.2 * rnd(E), 0.3 * nrm(E))  # a third pitched 70-140 degrees: past vertical
    wobble = torch.where(pick[:, None], torch.zeros(E, 3), 0.2 * nrm(E, 3))        # (a pitch about y itself keeps the chosen heading)
    pitch = quat(torch.tensor([0.0, 1.0, 0.0]).expand(E, 3) + wobble, pitch_a).double()
    root_rot = quat_mul(yaw, pitch)
    rb = torch.zeros(E, 24, 13, dtype=F64)
    rb[:, :, :3] = root_pos[:, None, :].double() + (nrm(E, 24, 3) * 0.45).double()
    rb[:, 0, :3] = root_pos.double()
    body_q = quat(nrm(E, 24, 3), nrm(E, 24) * 1.5).double()
    rb[:, :, 3:7] = quat_mul(root_rot[:, None, :].expand(E, 24, 4), body_q)
    rb[:, 0, 3:7] = root_rot
    rb[:, HEAD_BODY, :2] = rb[:, 0, :2] + 0.2 * nrm(E, 2).double()
    rb[:, :, 7:10] = (nrm(E, 24, 3) * 1.5).double()
    rb[:, :, 10:13] = (nrm(E, 24, 3) * 4.0).double()
    rb = rb.float()
    dof_state = torch.stack([nrm(E, 69) * 0.5, nrm(E, 69) * 3.0], dim=-1)
    dof_state[:, 0:3, 0] *= 0.01                                                  # a nearly straight joint (small rotation vector)
    dof_force = nrm(E, 69) * 40.0
    betas = nrm(E, 17)
    ml = int(max_episode_length)
    edge = torch.tensor([0, 1, 2, ml - 2, ml - 1, ml])
    progress = torch.where(k % 4 == 0, edge[(k // 4) % 6], (rnd(E) * (ml + 1)).long().clamp(max=ml))
    if E < 24:
        progress = edge[k % 6] if E >= 6 else progress
    # trajectory: a walk of ~1.2 m/s from near the root; a fifth of the envs starts 3-5.5 m away (both sides of the 4 m fail distance)
    dt, sample_dt = 1.0 / 30.0, 0.4
    vert_dt = ml * dt / 100.0
    head = (rnd(E) * 2.0 - 1.0) * math.pi
    step = torch.stack([torch.cos(head), torch.sin(head)], dim=1)[:, None, :] * (1.2 * vert_dt) + 0.01 * nrm(E, 101, 2)
    path = torch.cumsum(step, dim=1) - step[:, :1]
    off_r = torch.where(k % 5 == 2, 3.0 + 2.5 * rnd(E), 1.5 * rnd(E))
    off_a = (rnd(E) * 2.0 - 1.0) * math.pi
    verts = torch.zeros(E, 101, 3)
    verts[:, :, :2] = path
    # the offset is placed so that the sample at the env's own progress sits off_r from the root
    now = traj_calc_pos(verts, progress.double() * float(torch.tensor(dt, dtype=F32)), 101 * vert_dt)[:, :2].float()
    verts[:, :, :2] += (root_pos[:, :2] + torch.stack([off_r * torch.cos(off_a), off_r * torch.sin(off_a)], dim=1) - now)[:, None, :]
    verts[:, :, 2] = nrm(E, 101) * 0.01
    mask = torch.zeros(24, dtype=torch.uint8)
    mask[list(CONTACT_BODIES)] = 1
    cf = nrm(E, 24, 3) * 3.0
    cf[:, list(CONTACT_BODIES)] = nrm(E, 4, 3) * 400.0                             # the feet carry the weight and must not count
    want = 200.0 * rnd(E)                                                          # the unmasked sum's size: 0 .. 200 N
    want[::7] = 0.0
    live = (mask == 0).float()
    s = (cf * live[None, :, None]).sum(1)
    dirn = nrm(E, 3)
    dirn = dirn / dirn.norm(dim=-1, keepdim=True)
    cf[:, 11] += dirn * want[:, None] - s
    if E > 1:
        cf[::7] = 0.0
        cf[::7, list(CONTACT_BODIES)] = 300.0
    return dict(rb_state=rb, dof_state=dof_state, dof_force=dof_force, contact_force=cf, betas=betas, traj_verts=verts,
                progress=progress.long(), contact_body_mask=mask, dt=dt, sample_dt=sample_dt, traj_dur=101 * vert_dt,
                fail_dist=4.0, max_episode_length=float(ml), power_coef=0.0005)


def task_map(rows=520, cols=610, seed=3):
    """a non-square int16 height map (0.1 m cells, 0.005 m units): the envs of case_task stand 40-120 m out in every direction, so
    their probes leave it on all four sides (negative world coordinates included) and some stand on it; steps of up to +-4 m so that the
    +-3 clip of the height observations is reached"""
    g = _gen(seed)
    i, j = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    coarse = torch.randint(-800, 800, (rows // 8 + 1, cols // 8 + 1), generator=g)[i // 8, j // 8]
    fine = torch.randint(-3, 4, (rows, cols), generator=g)
    return (coarse + fine).to(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reset path (include/emloco_task.h: "Fused reset of finished envs"): every formula restated from the definitions the header
# cites (motion_lib_smpl.py:485-606, torch_utils.py slerp / quat_to_exp_map, humanoid_pedestrain_terrain.py:526-631,
# humanoid_amp.py:321-379), in the dtype given

GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX = 0, 1, 2
SLERP_C_STAR = math.sqrt(1.0 - 1e-6)         # the cosine at which slerp's sin(half angle) crosses 1e-3


def quat_apply(q, v):
    """quat_apply: v + w t + q_v x t with t = 2 q_v x v"""
    qv, w = q[..., :3], q[..., 3:4]
    qv, v = torch.broadcast_tensors(qv, v)
    t = torch.cross(qv, v, dim=-1) * 2.0
    return v + w * t + torch.cross(qv, t, dim=-1)


def frame_blend(time, length, dt, nframes, dtype=F64):
    """_calc_frame_blend: phase = clip(time / len, 0, 1); time = max(time, 0) AFTER the phase; i0 = trunc(phase (nf - 1)),
    i1 = min(i0 + 1, nf - 1); blend = (time - i0 dt) / dt, not clamped.  -> i0, i1 (int64), blend"""
    time, length, dt = _c(time, dtype), _c(length, dtype), _c(dt, dtype)
    nf = torch.as_tensor(nframes).to("cpu").long()
    phase = torch.clamp(time / length, 0.0, 1.0)
    time = torch.clamp_min(time, 0.0)
    i0 = (phase * (nf - 1).to(dtype)).long()
    i1 = torch.minimum(i0 + 1, nf - 1)
    return i0, i1, (time - i0.to(dtype) * dt) / dt


def slerp(q0, q1, t, dtype=F64):
    """torch_utils.slerp: q1 is flipped where the cosine is negative; the midpoint where |sin(half angle)| < 1e-3; q0 where
    |cos| >= 1; t broadcasts over the leading dimensions ([...] or [..., 1])"""
    q0, q1, t = _c(q0, dtype), _c(q1, dtype), _c(t, dtype)
    if t.dim() < q0.dim():
        t = t[..., None]
    c = (q0 * q1).sum(-1, keepdim=True)
    q1 = torch.where(c < 0, -q1, q1)
    c = c.abs()
    half = torch.acos(c)
    s = torch.sqrt(1.0 - c * c)
    out = (torch.sin((1.0 - t) * half) / s) * q0 + (torch.sin(t * half) / s) * q1
    out = torch.where(s.abs() < 0.001, 0.5 * q0 + 0.5 * q1, out)
    return torch.where(c.abs() >= 1.0, q0.expand_as(out), out)


def slerp_branch_distances(q0, q1):
    """float64 cosine of two frames and its distances to slerp's branch points: the sign flip (c = 0) and the midpoint / q0 branches
    (c = sqrt(1 - 1e-6) .. 1: one band, the two lie 5e-7 apart).  Frames that are equal or antipodal are on no branch: every branch
    returns q0 there."""
    q0, q1 = _c(q0, F64), _c(q1, F64)
    c = (q0 * q1).sum(-1)
    same = (q0 == q1).all(-1) | (q0 == -q1).all(-1)
    big = torch.full_like(c, 1e30)
    return torch.where(same, big, c.abs()), torch.where(same, big, (c.abs() - SLERP_C_STAR).abs().minimum((c.abs() - 1.0).abs()))


def quat_to_exp_map(q, dtype=F64):
    """torch_utils.quat_to_exp_map: sin = sqrt(1 - w^2), angle = 2 acos(w) wrapped through atan2(sin, cos); angle x q_v / sin where
    |sin| > 1e-5, zero elsewhere"""
    q = _c(q, dtype)
    w = q[..., 3:4]
    sin_theta = torch.sqrt(1.0 - w * w)
    angle = 2.0 * torch.acos(w)
    angle = torch.atan2(torch.sin(angle), torch.cos(angle))
    e = angle * (q[..., :3] / sin_theta)
    return torch.where(sin_theta.abs() > 1e-5, e, torch.zeros_like(e))


def motion_state(cache, mid, time, key_bodies=KEY_BODIES, dtype=F64):
    """get_motion_state_smpl on a motion cache (dict of gts / grs / lrs / gvs / gavs [F][24][.], dvs [F][69], motion_len / motion_dt /
    motion_nframes / motion_start [M]) for clip ids `mid` [n] at `time` [n] -> dict: root_pos / root_rot / root_vel / root_ang_vel,
    dof_pos / dof_vel [n][69], key_pos [n][4][3], local_rot [n][24][4] (the blended joint quaternions), f0 / f1 / blend"""
    mid = torch.as_tensor(mid).to("cpu").long()
    g = lambda k: torch.as_tensor(cache[k]).to("cpu")
    i0, i1, w = frame_blend(time, g("motion_len")[mid], g("motion_dt")[mid], g("motion_nframes")[mid], dtype=dtype)
    f0, f1 = i0 + g("motion_start")[mid].long(), i1 + g("motion_start")[mid].long()
    lerp = lambda a, wt: (1.0 - wt) * _c(a[f0], dtype) + wt * _c(a[f1], dtype)
    gts = lerp(g("gts"), w[:, None, None])
    lq = slerp(g("lrs")[f0], g("lrs")[f1], w[:, None], dtype=dtype)
    return dict(root_pos=gts[:, 0], root_rot=slerp(g("grs")[f0, 0], g("grs")[f1, 0], w, dtype=dtype),
                root_vel=lerp(g("gvs")[:, 0], w[:, None]), root_ang_vel=lerp(g("gavs")[:, 0], w[:, None]),
                dof_pos=quat_to_exp_map(lq[:, 1:], dtype=dtype).reshape(-1, 69), dof_vel=lerp(g("dvs"), w[:, None]),
                key_pos=gts[:, list(key_bodies)], local_rot=lq, f0=f0, f1=f1, blend=w)


def reset_pick(u, n):
    """min(trunc(u n), n - 1) with u n as the float32 product the launch forms (u and n are float32 numbers)"""
    u = torch.as_tensor(u).to("cpu").float()
    return torch.clamp((u * float(n)).long(), max=n - 1)


def reset_root(state, u_yaw, u_speed, random_heading, place_xy, dtype=F64):
    """the root of a reset from a motion_state: with random_heading the turn yaw = pi (2 u - 1) about z (hq x rot, hq applied to the angular
    velocity) and the forward speed 0.5 u + 1 in place of the x velocity, turned by the NEW heading; x, y are the placement
    -> xy [n][2], rot, vel, ang_vel"""
    rot, vel, ang = (_c(state[k], dtype).clone() for k in ("root_rot", "root_vel", "root_ang_vel"))
    if random_heading:
        yaw = math.pi * (2.0 * _c(u_yaw, dtype) - 1.0)
        hq = quat_about_z(yaw)
        rot = quat_mul(hq, rot)
        ang = quat_apply(hq, ang)
        vel = torch.cat([(_c(u_speed, dtype) * 0.5 + 1.0)[:, None], vel[:, 1:]], dim=1)
        vel = quat_apply(quat_about_z(calc_heading(rot)), vel)
    return _c(place_xy, dtype), rot, vel, ang


def rotvec_to_quat(e):
    """rotation vector -> unit quaternion (the simulator's joint convention: no wrap, no threshold beyond 0 / 0)"""
    a = e.norm(dim=-1, keepdim=True)
    k = torch.where(a > 1e-12, torch.sin(a / 2.0) / a.clamp_min(1e-300), torch.full_like(a, 0.5))
    return torch.cat([e * k, torch.cos(a / 2.0)], dim=-1)


def forward_kinematics(root_state, dof_pos, parent, joint_off, dtype=F64):
    """body positions [E][24][3] and rotations [E][24][4] of a tree (parent [24], joint_off [E][24][3]) from the root pose and the
    joints' rotation vectors [E][69]: p_b = p_parent + R_parent off_b, q_b = q_parent x q_joint"""
    rs, dp, off = _c(root_state, dtype), _c(dof_pos, dtype).reshape(-1, 23, 3), _c(joint_off, dtype)
    qj = rotvec_to_quat(dp)
    pos, rot = [rs[:, 0:3]], [rs[:, 3:7] / rs[:, 3:7].norm(dim=-1, keepdim=True)]
    for b in range(1, 24):
        p = int(parent[b])
        pos.append(pos[p] + quat_rotate(rot[p], off[:, b]))
        q = quat_mul(rot[p], qj[:, b - 1])
        rot.append(q / q.norm(dim=-1, keepdim=True))
    return torch.stack(pos, dim=1), torch.stack(rot, dim=1)


def lowest_collision_point(body_pos, body_rot, geom_type, geom_a, geom_b, geom_r, dtype=F64):
    """the lowest z over the simulator's ground-contact candidates: a sphere's centre (geom_a), a capsule's two ends (geom_a, geom_b), a
    box's eight corners (centre geom_a, half extents geom_b), in the body frame, each minus the body's radius geom_r -> [E]"""
    p, q, ga, gb, gr = (_c(t, dtype) for t in (body_pos, body_rot, geom_a, geom_b, geom_r))
    low = torch.full((p.shape[0],), float("inf"), dtype=dtype)
    for b in range(p.shape[1]):
        gt = int(geom_type[b])
        if gt == GEOM_SPHERE:
            pts = [ga[:, b]]
        elif gt == GEOM_CAPSULE:
            pts = [ga[:, b], gb[:, b]]
        else:
            sg = lambda k, bit: 1.0 if k & bit else -1.0
            pts = [ga[:, b] + gb[:, b] * torch.tensor([sg(k, 1), sg(k, 2), sg(k, 4)], dtype=dtype) for k in range(8)]
        for lp in pts:
            low = torch.minimum(low, p[:, b, 2] + quat_rotate(q[:, b], lp)[:, 2] - gr[:, b])
    return low


def _fmix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def reset_rnd_row(seed, bi, n=512):
    """row bi of the device's random rows for a 64-bit seed, exact (Python integers): per row fmix32(seed_lo ^ bi 0x9E3779B1) + seed_hi,
    per entry k two rounds of the murmur3 finaliser around + 0x165667B1; the top 24 bits over 2^24 (exact in float32)"""
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    row = (_fmix32(lo ^ ((bi * 0x9E3779B1) & 0xFFFFFFFF)) + hi) & 0xFFFFFFFF
    out = []
    for k in range(n):
        x = _fmix32((_fmix32(row ^ ((k * 0x27D4EB2F) & 0xFFFFFFFF)) + 0x165667B1) & 0xFFFFFFFF)
        out.append((x >> 8) / 16777216.0)
    return torch.tensor(out, dtype=F64).float()


def real_pick_perm(x, n, key):
    """the keyed bijection of [0, n) that picks a real path: 4-round Feistel network over the next even power of two >= n (at least 4),
    halves swapped each round with F = fmix32(r 0x9E3779B1 + key + round 0x85EBCA6B), cycle-walked until the value is below n"""
    bits = 2
    while (1 << bits) < n:
        bits += 2
    half = bits >> 1
    mask = (1 << half) - 1
    while True:
        l, r = x >> half, x & mask
        for rnd in range(4):
            l, r = r, l ^ (_fmix32((r * 0x9E3779B1 + key + rnd * 0x85EBCA6B) & 0xFFFFFFFF) & mask)
        x = (l << half) | r
        if x < n:
            return x


def seeded_real_key(seed):
    """the permutation key a seeded reset derives from its seed: the high word of seed x 0xD6E8FEB86659FD93 (mod 2^64)"""
    return ((seed * 0xD6E8FEB86659FD93) & 0xFFFFFFFFFFFFFFFF) >> 32


RESET_INIT_HEADING, RESET_HEADING_INVERSION, RESET_ADJUST_ROOT_VEL, RESET_REAL_PATH = 2, 4, 8, 16
RND_REAL, RND_INVERSION, RND_HEADING, RND_SPEED0, RND_DTHETA, RND_SHARP, RND_BERN, RND_DSPEED = 5, 7, 8, 9, 16, 116, 216, 316


def reset_trajectory(u, ip, rv, p, flags, real=None, real_rows=None, dtype=F64):
    """TrajGenerator.reset (traj_generator.py:60-237) for n list entries from their random rows u [n][512], start ip [n][2] and root
    velocity rv [n][3]; p: the scalar fields of EmlocoResetBufs by name (float32 numbers).  A clamped random walk of 100 segments (the
    first heading free, a sharp turn where the Bernoulli draw is below sharp_prob; with ADJUST_ROOT_VEL every segment's speed scaled by
    |rv_xy| / the first speed and clamped again); with REAL_PATH and u[RND_REAL] > hybrid_prob row real_rows[i] of real [R][101][3]
    instead, moved to ip (ADJUST_ROOT_VEL: scaled so that its first segment, at least speed_min vert_dt long, is |rv_xy| vert_dt);
    INIT_HEADING: turned about its start so that the first segment points along rv (plus pi where HEADING_INVERSION and
    u[RND_INVERSION] > 0.5; a zero velocity or a zero first segment counts as heading 0).  -> verts [n][101][3], inverted, is_real [n]"""
    u, ip, rv = _c(u, dtype), _c(ip, dtype), _c(rv, dtype)
    f = lambda k: torch.tensor(p[k], dtype=F32).to(dtype)
    vdt, smin, smax = f("vert_dt"), f("speed_min"), f("speed_max")
    pi = torch.tensor(math.pi, dtype=dtype)
    n = u.shape[0]
    adjust = bool(flags & RESET_ADJUST_ROOT_VEL)
    hv = torch.sqrt(rv[:, 0] * rv[:, 0] + rv[:, 1] * rv[:, 1])
    speed = (smax - smin) * u[:, RND_SPEED0] + smin
    ratio = hv / speed
    theta, px, py = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
    verts = torch.zeros(n, 101, 3, dtype=dtype)
    verts[:, 0, 0], verts[:, 0, 1] = ip[:, 0], ip[:, 1]
    for i in range(100):
        dth = (2.0 * u[:, RND_DTHETA + i] - 1.0) * (f("dtheta_max") * vdt)
        dth = torch.where(u[:, RND_BERN + i] < f("sharp_prob"), pi * (2.0 * u[:, RND_SHARP + i] - 1.0), dth)
        if i == 0:
            dth = pi * (2.0 * u[:, RND_HEADING] - 1.0)
        else:
            speed = torch.clamp(speed + (2.0 * u[:, RND_DSPEED + i] - 1.0) * (f("accel_max") * vdt), smin, smax)
        sp = torch.clamp(ratio * speed, smin, smax) if adjust else speed
        theta = theta + dth
        px, py = px + torch.cos(theta) * (sp * vdt), py - torch.sin(theta) * (sp * vdt)
        verts[:, i + 1, 0], verts[:, i + 1, 1] = px + ip[:, 0], py + ip[:, 1]
    is_real = torch.zeros(n, dtype=torch.bool)
    if (flags & RESET_REAL_PATH) and real is not None and real.shape[0] > 0:
        is_real = u[:, RND_REAL] > f("hybrid_prob")
        src = _c(real, dtype)[torch.as_tensor(real_rows).long()]
        sc = torch.ones(n, dtype=dtype)
        if adjust:
            first = torch.clamp_min((src[:, 1] - src[:, 0]).norm(dim=-1), smin * vdt)
            sc = hv / first * vdt
        moved = torch.cat([sc[:, None, None] * (src[:, :, :2] - src[:, :1, :2]) + ip[:, None, :], src[:, :, 2:]], dim=-1)
        verts = torch.where(is_real[:, None, None], moved, verts)
    inverted = torch.zeros(n, dtype=torch.bool)
    if flags & RESET_INIT_HEADING:
        o = verts[:, 0, :2].clone()
        d = verts[:, 1, :2] - o
        rmag, dmag = rv.norm(dim=-1), d.norm(dim=-1)
        zero = torch.zeros(n, dtype=dtype)
        root_rot = torch.where(rmag > 0, torch.atan2(rv[:, 1], rv[:, 0]), zero)
        ih = torch.where(dmag > 0, torch.atan2(d[:, 1], d[:, 0]), zero)
        if flags & RESET_HEADING_INVERSION:
            inverted = u[:, RND_INVERSION] > 0.5
        rd = torch.where(inverted, ih - root_rot + pi, ih - root_rot)
        c, s = torch.cos(rd)[:, None], torch.sin(rd)[:, None]
        x, y = verts[:, :, 0] - o[:, :1], verts[:, :, 1] - o[:, 1:]
        verts = torch.stack([(x * c + y * s) + o[:, :1], (-x * s + y * c) + o[:, 1:], verts[:, :, 2]], dim=-1)
    return verts, inverted, is_real
