"""Plain-torch restatement of the reference Solver's PPO update (agents/solver.py:141-204 with the
zero-hidden forward of networks.py:93-116), in float64 by default: GAE over one flat buffer,
unbiased-std advantage normalisation, epochs of shuffled minibatches, Categorical's probability
clamp, the clipped loss, clip_grad_norm_ and Adam.  Written from the reference's behaviour (no
text of it); tests/golden/solver_update_<case>.npz holds what the reference itself computed on
the same buffers, and the loaders for that fixture live here too.

    out = run_update(params, states, actions, old_logp, values, rewards, dones, perms, ...)

Nothing here touches a GPU or the package under test.
"""
import numpy as np
import torch
import torch.nn.functional as F

import golden_data as gd

CASES = ("g20", "g32", "g10", "clip20", "big20")
PARAMS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias",
          "fc_spatial.weight", "fc_spatial.bias", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0",
          "lstm.bias_hh_l0", "policy_head.0.weight", "policy_head.0.bias", "policy_head.2.weight",
          "policy_head.2.bias", "value_head.0.weight", "value_head.0.bias", "value_head.2.weight",
          "value_head.2.bias")  # SolverNetwork.parameters() order
N_CONV = 6  # the first six are stored in full, the rest as norm + projections
HH = PARAMS.index("lstm.weight_hh_l0")
SCALED = ("policy_head.2.weight", "value_head.2.weight")  # multiplied by a case's head_scale
F32_EPS = 1.1920929e-07  # Categorical(probs) clamps float32 probabilities to [eps, 1 - eps]
HYPER = dict(lr=3e-4, gamma=0.99, lam=0.95, clip=0.2, ecoef=0.05, vcoef=0.5, max_norm=0.5)


def proj_vectors(i, n, k=4):
    """The fixed projection vectors of parameter tensor i (tests/golden/make_golden.py)."""
    return np.random.default_rng(7000 + i).standard_normal((k, n))


# ---------------------------------------------------------------------------
# fixture
# ---------------------------------------------------------------------------

def pos_gradient(R, C):
    """The position channel's distance term (environment.py:361-365) as float32."""
    r, c = np.mgrid[0:R, 0:C]
    d = np.abs(r - (R - 2)) + np.abs(c - (C - 2))
    return (-0.3 * (d / (R + C))).astype(np.float32)


def encode_states(states, R, C):
    """[T, 3, R, C] float32 observations -> (occ [L, R*C] int8, lay [T] int16, vis [T, nb] uint8
    bits, pos [T] int16): the occupancy codes of each distinct layout, the layout of every
    state, the visibility bits and the Solver's flat position."""
    states = np.asarray(states, np.float32)
    occ_all = np.rint(states[:, 0] * 5).astype(np.int8).reshape(len(states), -1)
    occ, lay = np.unique(occ_all, axis=0, return_inverse=True)
    vis = np.packbits(states[:, 1].reshape(len(states), -1) > 0.5, axis=1)
    pos = (states[:, 2] - pos_gradient(R, C)[None]).reshape(len(states), -1).argmax(1)
    return occ, lay.reshape(-1).astype(np.int16), vis, pos.astype(np.int16)


def decode_states(occ, lay, vis, pos, R, C):
    """The float32 observations of encode_states' coding, bit for bit (environment.py:305-374:
    tile / 5, 0/1 visibility, 1 at the Solver and -1 at the vault plus the distance term)."""
    T = len(lay)
    s = np.empty((T, 3, R, C), np.float32)
    s[:, 0] = (occ[lay].astype(np.float32) / np.float32(5)).reshape(T, R, C)
    s[:, 1] = np.unpackbits(vis, axis=1)[:, :R * C].reshape(T, R, C).astype(np.float32)
    p = np.zeros((T, R * C), np.float32)
    p[np.arange(T), pos] = 1.0
    p[:, (R - 2) * C + (C - 2)] = -1.0
    s[:, 2] = p.reshape(T, R, C) + pos_gradient(R, C)[None]
    return s


def load_case(name):
    """One case of the fixture as a dict: decoded buffers, permutations, and the reference's
    recorded results (see make_golden.py make_solver_update for the keys)."""
    z = gd.load("solver_update_%s.npz" % name)
    c = {k: z[k] for k in z.files}
    R, C = int(c["cfg"][0]), int(c["cfg"][1])
    c.update(name=name, R=R, C=C, T=int(c["cfg"][2]), epochs=int(c["cfg"][3]), batch=int(c["cfg"][4]),
             head_scale=float(c["head_scale"]), rec_steps=[int(s) for s in c["rec_steps"]],
             n_steps=int(c["n_steps"]))
    c["states"] = decode_states(c["occ"], c["lay"], c["vis"], c["pos"], R, C)
    return c


def golden_params(head_scale=1.0, dtype=torch.float32):
    """The nets.npz Solver weights (SolverNetwork's parameters do not depend on the grid), the
    two head output layers multiplied by head_scale."""
    z = gd.load("nets.npz")
    sd = {k: torch.from_numpy(z["solver/" + k]).to(dtype) for k in PARAMS}
    for k in SCALED:
        sd[k] = sd[k] * head_scale
    return sd


def split_conv(flat):
    """The six conv tensors of a stored flat float32 vector, as float64 arrays."""
    shapes = ((32, 3, 3, 3), (32,), (64, 32, 3, 3), (64,), (64, 64, 3, 3), (64,))
    out, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(np.asarray(flat[o:o + n], np.float64).reshape(s))
        o += n
    assert o == len(flat)
    return out


# ---------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------

def gae(rewards, values, dones, gamma, lam):
    """agents/solver.py:228-244: backward recursion over one flat buffer, bootstrap 0 at its end."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last = rewards.new_zeros(())
    for t in range(T - 1, -1, -1):
        nxt = values[t + 1] if t + 1 < T else rewards.new_zeros(())
        live = 1 - dones[t]
        delta = rewards[t] + gamma * nxt * live - values[t]
        last = delta + gamma * lam * live * last
        adv[t] = last
    return adv


def forward(p, x, masks=None):
    """logits [B, A], values [B], and the three conv pre-activation signs (z > 0).  masks: three
    [B, ch, R, C] ReLU masks to use in place of the layers' own."""
    own, a = [], x
    for k in range(3):
        z = F.conv2d(a, p["conv%d.weight" % (k + 1)], p["conv%d.bias" % (k + 1)], padding=1)
        own.append(z.detach() > 0)
        a = z * (masks[k] if masks is not None else own[k]).to(z.dtype)
    f = F.adaptive_avg_pool2d(a, (4, 4)).reshape(x.shape[0], -1)
    s = F.relu(F.linear(f, p["fc_spatial.weight"], p["fc_spatial.bias"]))
    h0 = s.new_zeros(x.shape[0], p["lstm.weight_hh_l0"].shape[1])
    gates = (F.linear(s, p["lstm.weight_ih_l0"], p["lstm.bias_ih_l0"])
             + F.linear(h0, p["lstm.weight_hh_l0"], p["lstm.bias_hh_l0"]))
    i, f_, g, o = gates.chunk(4, dim=1)
    c1 = torch.sigmoid(f_) * 0 + torch.sigmoid(i) * torch.tanh(g)
    h1 = torch.sigmoid(o) * torch.tanh(c1)

    def head(n):
        return F.linear(F.relu(F.linear(h1, p[n + ".0.weight"], p[n + ".0.bias"])), p[n + ".2.weight"], p[n + ".2.bias"])
    return head("policy_head"), head("value_head").reshape(-1), own


def loss_parts(logits, values, actions, old_logp, adv, ret, clip):
    """(policy loss, value loss, entropy) of agents/solver.py:174-188."""
    probs = torch.softmax(logits, -1)
    probs = probs / probs.sum(-1, keepdim=True)
    logp_all = torch.log(probs.clamp(F32_EPS, 1 - F32_EPS))
    logp = logp_all.gather(1, actions[:, None])[:, 0]
    entropy = -(logp_all * probs).sum(-1).mean()
    ratio = torch.exp(logp - old_logp)
    pl = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    vl = ((values - ret) ** 2).mean()
    return pl, vl, entropy, ratio.detach()


def run_update(params, states, actions, old_logp, values, rewards, dones, perms, epochs, batch,
               record=(), masks=None, dtype=torch.float64, keep_signs=False, hyper=HYPER, stop_after=None):
    """The whole update from `params` (name -> tensor).  perms: [epochs, T] the shuffles.
    record: steps whose pre-clip gradients are kept.  masks: {step: three ReLU masks} forced on
    the conv layers of those steps.  stop_after: run that many steps only.  Returns a dict: adv (normalised), ret, metrics (policy,
    value, entropy: means over the steps), n_steps, steps {step: grads, total_norm, parts, ratio},
    params (after), signs (keep_signs: per step the three z > 0 tensors)."""
    h = hyper
    p = {k: params[k].detach().to(dtype).clone().requires_grad_() for k in PARAMS}
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    x_all, olp, val, rew, don = t(states), t(old_logp), t(values), t(rewards), t(dones)
    act = torch.as_tensor(np.asarray(actions)).long()
    T = x_all.shape[0]
    adv = gae(rew, val, don, h["gamma"], h["lam"])
    ret = adv + val
    if T > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    tot = np.zeros(3)
    step, steps, signs = 0, {}, []
    for e in range(epochs):
        idx = torch.as_tensor(np.asarray(perms[e])).long()
        for start in range(0, T, batch):
            if stop_after is not None and step >= stop_after:
                break
            b = idx[start:start + batch]
            logits, nv, own = forward(p, x_all[b], None if masks is None else masks.get(step))
            pl, vl, ent, ratio = loss_parts(logits, nv, act[b], olp[b], adv[b], ret[b], h["clip"])
            loss = pl + h["vcoef"] * vl - h["ecoef"] * ent
            grads = dict(zip(PARAMS, torch.autograd.grad(loss, [p[k] for k in PARAMS])))
            total = torch.stack([g.norm() for g in grads.values()]).norm()
            if step in record:
                steps[step] = dict(grads={k: g.clone() for k, g in grads.items()}, total_norm=float(total),
                                   parts=np.array([pl.item(), vl.item(), ent.item()]), ratio=ratio)
            if keep_signs:
                signs.append(own)
            coef = min(1.0, h["max_norm"] / (float(total) + 1e-6))
            step += 1
            with torch.no_grad():
                for k in PARAMS:
                    g = grads[k] * coef
                    m[k].mul_(0.9).add_(g, alpha=0.1)
                    v2[k].mul_(0.999).addcmul_(g, g, value=0.001)
                    denom = v2[k].sqrt() / (1 - 0.999 ** step) ** 0.5 + 1e-8
                    p[k].addcdiv_(m[k], denom, value=-h["lr"] / (1 - 0.9 ** step))
            tot += [pl.item(), vl.item(), ent.item()]
    return dict(adv=adv, ret=ret, metrics=tot / max(step, 1), n_steps=step, steps=steps,
                params={k: v.detach() for k, v in p.items()}, signs=signs)


# ---------------------------------------------------------------------------
# comparisons shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------

def rel_max(got, want):
    """max |got - want| relative to max |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want)) / max(float(np.linalg.norm(want)), 1e-300)


def check_tensors(got, conv, norms, projs, bound, what, conv_metric=rel_max, proj_factor=4.0, full=None):
    """got: the 20 tensors (float64 numpy, PARAMS order) against a stored record: the six conv
    tensors in full (conv_metric <= bound[i]), the others by L2 norm (rtol bound[i]) and their 4
    projections (within proj_factor * bound[i] * norm: 4 for gradients, tests/test_architect_update.py's
    4e-4 x norm beside 1e-4; 1 for the parameter change); lstm.weight_hh_l0 exactly zero.  bound: one
    number or one per tensor.  full: {index: (stored tensor, allowed |difference| per element)} for
    tensors held element by element instead (measured: the worst difference / allowed, bound 1).
    Returns ({name: measured}, [(name, measured, bound) over the bound]); measured is the metric for
    conv tensors, else the larger of the norm's relative error and the worst projection error /
    (proj_factor * norm)."""
    bound = np.broadcast_to(np.asarray(bound, np.float64), (len(PARAMS),)).copy()
    want_conv = split_conv(conv)
    seen, bad = {}, []
    for i, name in enumerate(PARAMS):
        g = np.asarray(got[i], np.float64)
        if i == HH:
            assert not g.any(), "%s %s: not exactly zero" % (what, name)
            continue
        if full is not None and i in full:
            want, allowed = full[i]
            seen[name] = float((np.abs(g.reshape(-1) - want.reshape(-1)) / allowed.reshape(-1)).max())
            bound[i] = 1.0
        elif i < N_CONV:
            seen[name] = conv_metric(g, want_conv[i])
        else:
            n = float(norms[i])
            e_n = abs(float(np.linalg.norm(g)) - n) / max(n, 1e-300)
            e_p = float(np.abs(proj_vectors(i, g.size) @ g.reshape(-1) - projs[i]).max()) / max(proj_factor * n, 1e-300)
            seen[name] = max(e_n, e_p)
        if not seen[name] <= bound[i]:
            bad.append((name, seen[name], float(bound[i])))
    return seen, bad


def coarse_delta(c, p0, spacings):
    """For a case whose two head output layers were scaled up (|w| ~ 1e2 .. 3e3): float32 cannot
    resolve their Adam steps (lr 3e-4 against a spacing of up to 2.4e-4), so their parameter change
    is quantised and a relative-L2 floor says nothing.  They are stored in full (d_heads) and held
    element by element: {index: (stored change, allowed)} with allowed = `spacings` float32
    spacings at that weight, plus 1e-4 of the largest change (the bound every other tensor's
    arithmetic has).  None for a case without scaling."""
    if "d_heads" not in c:
        return None
    out, o = {}, 0
    big = float(np.abs(c["d_heads"]).max())
    for k in SCALED:
        w = np.abs(p0[k].detach().cpu().numpy().astype(np.float32)).reshape(-1)
        want = np.asarray(c["d_heads"][o:o + w.size], np.float64)
        o += w.size
        spacing = np.spacing(w + np.float32(big)).astype(np.float64)  # the weight moves by <= big
        out[PARAMS.index(k)] = (want, spacings * spacing + 1e-4 * big)
    return out
