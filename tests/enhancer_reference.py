"""The Enhancer stage by stage in plain torch, dtype-generic: float64 is the truth of the kernel tests (test_gpu_enhancer_kernels.py), the
same code in float32 on the CPU their yardstick. Written from the operation (Enhancer_block with the attention commented out, FRFN,
SplitAttn with radix 1: enhancer.py:346-357, :222-250, :315-333); test_enhancer_reference.py pins it against oracle/torch_port.py, the
golden fixtures and a hand-computed border pixel.

Every stage takes its INPUT as an argument (the kernel tests hand in what the kernel actually read, cast to float64, so a bound is per
stage) and the parameters as a state dict with the Enhancer's own keys (the names of _lib.enhancer_param_table). Intermediates are
token-major [n, H, W, channels], as the kernels keep them:
  K1  ln(sd, x)            x [n, C, H, W]      -> Y = x + LN1(x), Zln = LN2(Y)
  K2  pconv(sd, Zln)       3x3 convolution without bias on the first C / 4 channels, the others untouched -> Z
  K3  linear1(sd, Z)       GELU(Z W1^T + b1)   -> Hd [.., 4C]: x1 = Hd[.., :2C], x2 = Hd[.., 2C:]
  K4  dwgate(sd, Hd)       GELU(depthwise 3x3(x1) + bias) * x2 -> G [.., 2C]; the convolution pads x1 = GELU(.) with ZEROS
  K5  linear2(sd, G, Y)    G W2^T + b2 + Y     -> O;  colsum = O summed over the pixels
  K6  gate(sd, colsum, HW) sigmoid(fc2 ReLU(LN(fc1 colsum / HW))) -> [n, C]
  K7  scale_out(O, gate)   O * gate, channels first -> out [n, C, H, W]"""
import numpy as np
import torch
import torch.nn.functional as F

P1, PM, PS = "block_1.", "block_1.mlp.", "split_attn."
KEYS = (P1 + "norm1.weight", P1 + "norm1.bias", P1 + "norm2.weight", P1 + "norm2.bias", PM + "partial_conv3.weight",
        PM + "linear1.0.weight", PM + "linear1.0.bias", PM + "dwconv.0.weight", PM + "dwconv.0.bias", PM + "linear2.0.weight",
        PM + "linear2.0.bias", PS + "fc1.weight", PS + "bn1.weight", PS + "bn1.bias", PS + "fc2.weight")


def cast(sd, dt):
    return {k: sd[k].to(dt) for k in KEYS}


def ln(sd, x):
    C = x.shape[1]
    t = x.permute(0, 2, 3, 1)
    Y = t + F.layer_norm(t, (C,), sd[P1 + "norm1.weight"], sd[P1 + "norm1.bias"], eps=1e-5)
    return Y, F.layer_norm(Y, (C,), sd[P1 + "norm2.weight"], sd[P1 + "norm2.bias"], eps=1e-5)


def pconv(sd, Zln):
    dc = Zln.shape[-1] // 4
    head = F.conv2d(Zln[..., :dc].permute(0, 3, 1, 2), sd[PM + "partial_conv3.weight"], None, padding=1).permute(0, 2, 3, 1)
    return torch.cat([head, Zln[..., dc:]], dim=-1)


def linear1(sd, Z):
    return F.gelu(F.linear(Z, sd[PM + "linear1.0.weight"], sd[PM + "linear1.0.bias"]))


def dwgate(sd, Hd):
    hid = Hd.shape[-1] // 2
    x1 = Hd[..., :hid].permute(0, 3, 1, 2)
    d = F.conv2d(x1, sd[PM + "dwconv.0.weight"], sd[PM + "dwconv.0.bias"], padding=1, groups=hid)   # zero padding of GELU(x1)
    return F.gelu(d).permute(0, 2, 3, 1) * Hd[..., hid:]


def linear2(sd, G, Y):
    return F.linear(G, sd[PM + "linear2.0.weight"], sd[PM + "linear2.0.bias"]) + Y


def gate(sd, colsum, HW):
    C = colsum.shape[-1]
    g = F.linear(colsum / HW, sd[PS + "fc1.weight"])
    g = F.relu(F.layer_norm(g, (C,), sd[PS + "bn1.weight"], sd[PS + "bn1.bias"], eps=1e-5))
    return torch.sigmoid(F.linear(g, sd[PS + "fc2.weight"]))


def scale_out(O, gt):
    return (O * gt[:, None, None, :]).permute(0, 3, 1, 2).contiguous()


def forward(sd, x, dt=torch.float64):
    """Every intermediate of the module in dtype dt: Y, Zln, Z, Hd (x1 | x2), G, O, colsum, mean, gate, out."""
    sd, x = cast(sd, dt), x.to(dt)
    r = {}
    r["Y"], r["Zln"] = ln(sd, x)
    r["Z"] = pconv(sd, r["Zln"])
    r["Hd"] = linear1(sd, r["Z"])
    hid = r["Hd"].shape[-1] // 2
    r["x1"], r["x2"] = r["Hd"][..., :hid], r["Hd"][..., hid:]
    r["G"] = dwgate(sd, r["Hd"])
    r["O"] = linear2(sd, r["G"], r["Y"])
    r["colsum"] = r["O"].sum((1, 2))
    HW = x.shape[2] * x.shape[3]
    r["mean"] = r["colsum"] / HW
    r["gate"] = gate(sd, r["colsum"], HW)
    r["out"] = scale_out(r["O"], r["gate"])
    return r


def random_sd(C, seed, bias1=1.0):
    """float32 parameters of ordinary size: unit-variance pre-activations, LayerNorm affines around (1, 0), a Linear1 bias of order bias1
    (so that GELU(bias) is far from 0: the depthwise stage's zero padding and a GELU(bias) padding differ)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    dc, hid = C // 4, 2 * C
    return {P1 + "norm1.weight": 1 + 0.3 * r(C), P1 + "norm1.bias": 0.3 * r(C), P1 + "norm2.weight": 1 + 0.3 * r(C), P1 + "norm2.bias": 0.3 * r(C),
            PM + "partial_conv3.weight": r(dc, dc, 3, 3) / (9 * dc) ** 0.5,
            PM + "linear1.0.weight": r(2 * hid, C) / C ** 0.5, PM + "linear1.0.bias": bias1 * r(2 * hid),
            PM + "dwconv.0.weight": r(hid, 1, 3, 3) / 3.0, PM + "dwconv.0.bias": 0.5 * r(hid),
            PM + "linear2.0.weight": r(C, hid) / hid ** 0.5, PM + "linear2.0.bias": r(C),
            PS + "fc1.weight": r(C, C) / C ** 0.5, PS + "bn1.weight": 1 + 0.3 * r(C), PS + "bn1.bias": 0.3 * r(C), PS + "fc2.weight": r(C, C) / C ** 0.5}


def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-300))


def subsets(n, H, W, tw, th):
    """Named boolean masks [n, H, W] over which an error is judged separately, so that a wrong edge is not averaged away: the image's
    border ring, the pixels of the last partial tile column (tw-pixel tiles) and row (th), each agent."""
    m = {}
    ring = torch.zeros(n, H, W, dtype=torch.bool)
    ring[:, 0], ring[:, -1], ring[:, :, 0], ring[:, :, -1] = True, True, True, True
    m["border ring"] = ring
    if W % tw:
        lx = torch.zeros(n, H, W, dtype=torch.bool)
        lx[:, :, W - W % tw:] = True
        m[f"last partial tile in x ({tw})"] = lx
    if H % th:
        ly = torch.zeros(n, H, W, dtype=torch.bool)
        ly[:, H - H % th:] = True
        m[f"last partial tile in y ({th})"] = ly
    if n > 1:
        for a in range(n):
            ag = torch.zeros(n, H, W, dtype=torch.bool)
            ag[a] = True
            m[f"agent {a}"] = ag
    return m
