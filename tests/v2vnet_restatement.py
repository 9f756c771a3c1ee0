"""Torch restatements of V2VNet fusion in any dtype, the fixture's case table and its poses. Shared by tests/test_v2vnet.py,
tests/test_gpu_v2vnet.py, tools/make_golden_v2vnet.py and tools/v2vnet_bench.py. Framework operators only: nothing here touches the HIP
library.

``v2vnet_forward`` is the DECOMPOSED algorithm gencomm_amd/v2vnet.py runs, written from three equivalences:
  1. a convolution over concatenated channels is the sum of the convolutions of the parts, so the message convolution of
     cat[warped source, node] splits into a source term (per pair) and a node term + bias (per node);
  2. a ConvGRU cell whose hidden state is zero: the reset gate multiplies zeros, the hidden-state input columns multiply zeros, and
     (1 - u) 0 + u tanh(candidate) = sigmoid(beta) tanh(candidate) with beta the second half of the gate convolution's rows;
  3. only node 0 of the last round is returned, so the last round updates node 0 of every scene only.
``v2vnet_loop_forward`` is the undecomposed loop (every node in every round, concatenated inputs, full weights, explicit zero state): the
orientation figure of tools/v2vnet_bench.py and a second opinion in the tests."""
import numpy as np
import torch
import torch.nn.functional as F

RECORD_LEN = [2, 3, 1, 4]
L = 5
# the fixture's configurations (tools/make_golden_v2vnet.py); `data` names the stored input and poses (a, b and c share theirs)
CASES = {
    "a": dict(C=8, H=12, W=20, agg="avg", gru=True, layers=1, iters=2, data="a"),
    "b": dict(C=8, H=12, W=20, agg="max", gru=True, layers=2, iters=3, data="a"),
    "c": dict(C=8, H=12, W=20, agg="avg", gru=False, layers=1, iters=1, data="a"),
    "d": dict(C=32, H=8, W=12, agg="avg", gru=True, layers=1, iters=2, data="d"),   # every convolution on the three-term matrix-pipe route
}


def case_args(c):
    return {"in_channels": c["C"], "num_iteration": c["iters"], "gru_flag": c["gru"], "agg_operator": c["agg"],
            "conv_gru": {"H": c["H"], "W": c["W"], "num_layers": c["layers"], "kernel_size": [[3, 3]] * c["layers"]}}


def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-300))


def make_affine(record_len, max_cav, H, W, seed, off_map=None):
    """Normalised pairwise matrices [B, L, L, 2, 3] float64 with EVERY row filled: synth.make_pairwise_t_matrix (shifts up to 0.3 W
    pixels, any yaw) -> normalize_pairwise_tfm at one pixel per metre. `off_map` = (scene, agent): that agent is moved 6 W pixels away
    and the scene's matrices are rebuilt from the world poses, so every pair with it misses the map and its mask is zero everywhere."""
    from gencomm_amd import normalize_pairwise_tfm, synth
    ptm = synth.make_pairwise_t_matrix(record_len, max_cav, seed, max_shift=0.3 * W)
    if off_map is not None:
        b, a = off_map
        n = record_len[b]
        world = [ptm[b, i, 0].copy() for i in range(n)]     # agent i's frame -> the ego's = the world's
        world[a][0, 3] += 6.0 * W
        for i in range(n):
            for j in range(n):
                ptm[b, i, j] = np.linalg.solve(world[j], world[i]) if i != j else np.eye(4)
    return normalize_pairwise_tfm(torch.from_numpy(ptm), H, W, 1.0).numpy()


def make_x(n, C, H, W, seed):
    """Post-ReLU-looking maps (half the entries zero), the egos included."""
    return np.maximum(np.random.RandomState(seed).standard_normal((n, C, H, W)), 0.0).astype(np.float32)


def warp(src, M):
    """warp_affine_simple: float64 affine grid cast to the input's dtype, bilinear, zeros, align_corners=False."""
    n, C, H, W = src.shape
    grid = F.affine_grid(M.to(torch.float64), [n, C, H, W], align_corners=False).to(src)
    return F.grid_sample(src, grid, align_corners=False)


def gate(g):
    """[n, 2C, ...] -> sigmoid(first half) * tanh(second half)."""
    C = g.shape[1] // 2
    return torch.sigmoid(g[:, :C]) * torch.tanh(g[:, C:])


def aggregate(y, e, h, theta, node_row, pair_off, op, out_mode):
    """The contract of gencomm_v2v_aggregate_fwd in torch: y [P, C, H, W], e [n_nodes, C, H, W], h [rows, C, H, W]."""
    P, C, H, W = y.shape
    mask = warp(torch.ones(P, 1, H, W, dtype=y.dtype), theta)
    out = []
    for k, row in enumerate(node_row):
        a, b = pair_off[k], pair_off[k + 1]
        m = (y[a:b] + e[k:k + 1]) * mask[a:b]
        agg = m.mean(0) if op == 0 else m.max(0)[0]
        out.append(torch.cat([h[row], agg], 0) if out_mode == 0 else h[row] + agg)
    return torch.stack(out)


def v2vnet_forward(sd, args, x, record_len, affine):
    """The decomposed forward in x's dtype; sd = a state dict with the reference's keys."""
    dt = x.dtype
    p = {k: v.detach().to(dt) for k, v in sd.items()}
    C = args["in_channels"]
    w_src, w_node = p["msg_cnn.weight"][:, :C], p["msg_cnn.weight"][:, C:]
    cells = []
    for l in range(args["conv_gru"]["num_layers"]):
        cin = 2 * C if l == 0 else C
        pre = f"conv_gru.cell_list.{l}."
        cells.append((torch.cat([p[pre + "conv_gates.weight"][C:, :cin], p[pre + "conv_can.weight"][:, :cin]], 0),
                      torch.cat([p[pre + "conv_gates.bias"][C:], p[pre + "conv_can.bias"]], 0)))
    off = np.concatenate([[0], np.cumsum(record_len)]).tolist()
    h = x
    for it in range(args["num_iteration"]):
        last = it == args["num_iteration"] - 1
        new = []
        for b, n in enumerate(record_len):
            hb = h[off[b]:off[b + 1]]
            for i in range(1 if last else n):
                th = affine[b, i, :n]
                y = F.conv2d(warp(hb, th), w_src, None, padding=1)
                e = F.conv2d(hb[i:i + 1], w_node, p["msg_cnn.bias"], padding=1)
                m = (y + e) * warp(torch.ones(n, 1, *x.shape[2:], dtype=dt), th)
                agg = m.mean(0) if args["agg_operator"] == "avg" else m.max(0)[0]
                if not args["gru_flag"]:
                    new.append(hb[i] + agg)
                    continue
                s = torch.cat([hb[i], agg], 0)[None]
                for w, bias in cells:
                    s = gate(F.conv2d(s, w, bias, padding=w.shape[-1] // 2))
                new.append(s[0])
        h = torch.stack(new)
    return F.linear(h.permute(0, 2, 3, 1), p["mlp.weight"], p["mlp.bias"]).permute(0, 3, 1, 2)


def v2vnet_loop_forward(sd, args, x, record_len, affine):
    """The undecomposed loop: every node in every round, concatenated inputs, full weights, an explicit zero hidden state."""
    dt = x.dtype
    p = {k: v.detach().to(dt) for k, v in sd.items()}
    C = args["in_channels"]
    H, W = x.shape[2:]
    off = np.concatenate([[0], np.cumsum(record_len)]).tolist()
    feats = [x[off[b]:off[b + 1]] for b in range(len(record_len))]
    for _ in range(args["num_iteration"]):
        nxt = []
        for b, n in enumerate(record_len):
            upd = []
            for i in range(n):
                th = affine[b, i, :n]
                nb = torch.cat([warp(feats[b], th), feats[b][i][None].repeat(n, 1, 1, 1)], 1)
                m = F.conv2d(nb, p["msg_cnn.weight"], p["msg_cnn.bias"], padding=1) * warp(torch.ones(n, 1, H, W, dtype=dt, device=x.device), th)
                agg = m.mean(0) if args["agg_operator"] == "avg" else m.max(0)[0]
                if not args["gru_flag"]:
                    upd.append(feats[b][i] + agg)
                    continue
                s = torch.cat([feats[b][i], agg], 0)[None]
                for l in range(args["conv_gru"]["num_layers"]):
                    pre = f"conv_gru.cell_list.{l}."
                    wg, wc = p[pre + "conv_gates.weight"], p[pre + "conv_can.weight"]
                    hc = torch.zeros(1, C, H, W, dtype=dt, device=x.device)
                    g = F.conv2d(torch.cat([s, hc], 1), wg, p[pre + "conv_gates.bias"], padding=wg.shape[-1] // 2)
                    r, u = torch.sigmoid(g[:, :C]), torch.sigmoid(g[:, C:])
                    cand = torch.tanh(F.conv2d(torch.cat([s, r * hc], 1), wc, p[pre + "conv_can.bias"], padding=wc.shape[-1] // 2))
                    s = (1 - u) * hc + u * cand
                upd.append(s[0])
            nxt.append(torch.stack(upd))
        feats = nxt
    out = torch.stack([f[0] for f in feats])
    return F.linear(out.permute(0, 2, 3, 1), p["mlp.weight"], p["mlp.bias"]).permute(0, 3, 1, 2)
