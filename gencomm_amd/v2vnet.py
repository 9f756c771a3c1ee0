"""``V2VNetFusion`` -- host-side mirror of the reference's V2VNet fusion (``opencood/models/fuse_modules/fusion_in_one.py:238-353`` with
``opencood/models/sub_modules/convgru.py``), the block ``v2vnet:`` of the ``*_v2vnet.yaml`` configs. Same constructor keys
(``in_channels, num_iteration, gru_flag, agg_operator, conv_gru: {H, W, num_layers, kernel_size}``), same ``forward(x, record_len,
affine_matrix)`` and the same ``state_dict`` keys, order and full shapes (``tests/golden/v2vnet_keys.json``), so a reference checkpoint
loads with ``strict=True``.

V2VNet is a graph network: in every one of ``num_iteration`` rounds each agent i of a scene receives a message from each agent j of the
scene (itself included), warped into i's frame by ``affine_matrix[b, i, j]`` -- every row of the pairwise matrix is read, not only the ego's.
The reference computes, per node, ``msg_cnn(cat[warp_ij(h_j), h_i]) * warp_ij(ones)``, the mean or max over j, and a ConvGRU on
``cat[h_i, agg]``. Three exact simplifications carry the HIP path:

  1. ``msg_cnn`` splits: conv(warp_ij(h_j); W[:, :C]) + conv(h_i; W[:, C:]) + bias. The second term is computed once per node; the 2C map
     is never formed.
  2. The ConvGRU is called with one time step and no hidden state, so ``h_cur = 0``: the reset gate and the hidden-state columns of both
     weight tensors multiply zeros, and ``h_next = sigmoid(beta) * tanh(candidate)`` with ``beta`` the SECOND half of ``conv_gates``'
     output channels. A cell is one convolution Cin -> 2C (rows [C:2C] of ``conv_gates`` over all rows of ``conv_can``, first Cin input
     columns) and a gate. THE HIDDEN-STATE COLUMNS AND THE RESET-GATE ROWS STAY IN THE STATE DICT, for the checkpoint's sake, ALTHOUGH
     THE FORWARD NEVER READS THEM.
  3. Only node 0 of the last round is returned, so the last round updates the ego nodes only.

Per round, all scenes batched:
  warp of all (i, j) pairs      gencomm_v2v_warp_pairs_fwd (a source map is read in place for each of its targets)
  source half of msg_cnn        gencomm_conv2d_fwd over the P warped maps, C -> C
  node half of msg_cnn + bias   gencomm_conv2d_fwd over the updated nodes, C -> C
  mask, mean / max, [h | agg]   gencomm_v2v_aggregate_fwd (the region-of-interest mask is evaluated in the kernel, never stored)
  per GRU layer                 gencomm_conv2d_fwd with the stacked [beta; candidate] weights, then gencomm_gru_gate_fwd
and ``mlp`` on the ego states as a 1x1 convolution. The sliced and stacked weights are prepared once and rebuilt only when a source
parameter changed (``optimizer.step()``, ``load_state_dict``).

Inference only: a call with gradients enabled into a module that has a parameter or an input requiring grad raises
``NotImplementedError`` (the backward of the three kernels is a follow-up).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .bev_backbone import _versions
from .fusion import MAX_AGENTS_PER_SCENE
from .runtime import conv2d_prepare, dev_ints, f32c, ptr, record_len_list, require_gpu, stream_ptr

AGG_OPERATORS = ("avg", "max")
KERNEL_SIZES = ((3, 3), (1, 1))     # what the ConvGRU cells are built for here


# ----------------------------------------------------------------------------------------- parameter containers
class ConvGRUCell(nn.Module):  # convgru.py:7-42
    def __init__(self, input_dim, hidden_dim, kernel_size):
        super().__init__()
        self.input_dim, self.hidden_dim = input_dim, hidden_dim
        pad = (kernel_size[0] // 2, kernel_size[1] // 2)
        self.conv_gates = nn.Conv2d(input_dim + hidden_dim, 2 * hidden_dim, kernel_size, padding=pad)   # [reset (gamma); update (beta)]
        self.conv_can = nn.Conv2d(input_dim + hidden_dim, hidden_dim, kernel_size, padding=pad)


class ConvGRU(nn.Module):  # convgru.py:73-127
    def __init__(self, input_dim, hidden_dim, kernel_sizes):
        super().__init__()
        self.cell_list = nn.ModuleList([ConvGRUCell(input_dim if i == 0 else hidden_dim, hidden_dim, k) for i, k in enumerate(kernel_sizes)])


def _kernel_sizes(conv_gru):
    ks, layers = conv_gru["kernel_size"], int(conv_gru["num_layers"])
    if layers < 1:
        raise ValueError(f"V2VNetFusion: conv_gru.num_layers {layers} is not supported (at least one layer)")
    if not isinstance(ks, list):                          # convgru.py:192-196: anything but a list is one size for every layer
        ks = [ks] * layers
    if len(ks) != layers:
        raise ValueError(f"V2VNetFusion: conv_gru.kernel_size has {len(ks)} entries for conv_gru.num_layers {layers}")
    out = []
    for k in ks:
        k = tuple(int(v) for v in k) if isinstance(k, (list, tuple)) else (int(k), int(k))
        if k not in KERNEL_SIZES:
            raise NotImplementedError(f"V2VNetFusion: conv_gru.kernel_size entry {list(k)} is not supported (the ConvGRU cells run as "
                                      f"[3, 3] or [1, 1] convolutions)")
        out.append(k)
    return out


# ----------------------------------------------------------------------------------------- the module
class V2VNetFusion(nn.Module):
    def __init__(self, args):
        super().__init__()
        C = self.in_channels = int(args["in_channels"])
        self.H, self.W = int(args["conv_gru"]["H"]), int(args["conv_gru"]["W"])
        self.num_iteration = int(args["num_iteration"])
        self.gru_flag = bool(args["gru_flag"])
        self.agg_operator = args["agg_operator"]
        if self.agg_operator not in AGG_OPERATORS:
            raise ValueError(f"V2VNetFusion: agg_operator {self.agg_operator!r} is not supported (one of {AGG_OPERATORS})")
        if self.num_iteration < 1:
            raise ValueError(f"V2VNetFusion: num_iteration {self.num_iteration} is not supported (at least one round)")
        self.kernel_sizes = _kernel_sizes(args["conv_gru"])
        self.msg_cnn = nn.Conv2d(C * 2, C, kernel_size=3, stride=1, padding=1)
        self.conv_gru = ConvGRU(C * 2, C, self.kernel_sizes)
        self.mlp = nn.Linear(C, C)
        self._prepared = {}

    # ---- kernel-layout weights, rebuilt only when a source parameter changed
    def _weights(self, key, sources, make, k, device):
        """`make()` -> (weight [Cout, Cin, k, k], bias [Cout] or None); returns (prepared, scale/shift rows, Cin, Cout, k)."""
        ver = _versions(*sources) + (str(device),)
        hit = self._prepared.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1:]
        w, b = make()
        w = f32c(w.detach())
        cout, cin = w.shape[:2]
        prepared = conv2d_prepare(w, cin, cout, k, k, 0, device)
        ss = torch.empty(2, cout, dtype=torch.float32, device=device)
        bb = f32c(b.detach()) if b is not None else None
        _lib.check(_lib.lib().gencomm_conv2d_fold(None, None, None, None, ptr(bb), 0.0, cout, ptr(ss[0]), ptr(ss[1]), stream_ptr(device)),
                   "gencomm_conv2d_fold")
        self._prepared[key] = (ver, prepared, ss, cin, cout, k)
        return prepared, ss, cin, cout, k

    @staticmethod
    def _conv(x, entry):
        prepared, ss, cin, cout, k = entry
        n, c, H, W = x.shape
        assert c == cin, (c, cin)
        y = torch.empty(n, cout, H, W, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().gencomm_conv2d_fwd(ptr(x), ptr(prepared), ptr(ss[0]), ptr(ss[1]), ptr(y), n, cin, H, W, cout, k, k, 1, k // 2, 0, 1,
                                                 cout, 0, stream_ptr(x.device)), "gencomm_conv2d_fwd")
        return y

    def _cell_weights(self, layer, device):
        cell = self.conv_gru.cell_list[layer]
        C, cin, k = cell.hidden_dim, cell.input_dim, self.kernel_sizes[layer][0]
        g, c = cell.conv_gates, cell.conv_can
        return self._weights(("cell", layer), [g.weight, g.bias, c.weight, c.bias],
                             lambda: (torch.cat([g.weight[C:, :cin], c.weight[:, :cin]], 0), torch.cat([g.bias[C:], c.bias], 0)), k, device)

    def forward(self, x, record_len, affine_matrix):
        """x [sumN, C, H, W], record_len [B], affine_matrix [B, L, L, 2, 3] -> [B, C, H, W]."""
        lens = record_len_list(record_len)
        n, C, H, W = x.shape
        B, L = affine_matrix.shape[:2]
        if len(lens) != B or sum(lens) != n or min(lens) < 1 or max(lens) > L:
            raise ValueError(f"record_len {lens} inconsistent with {n} agents / {B} scenes (1..{L} agents per scene)")
        if max(lens) > MAX_AGENTS_PER_SCENE:
            raise ValueError(f"each scene needs 1..{MAX_AGENTS_PER_SCENE} agents, got {lens}")
        if C != self.in_channels:
            raise ValueError(f"V2VNetFusion: input has {C} channels, the module was built with in_channels {self.in_channels}")
        if (H, W) != (self.H, self.W):
            raise ValueError(f"V2VNetFusion: input map is {H}x{W}, the module was built with conv_gru.H, conv_gru.W = {self.H}x{self.W}")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("v2vnet training is not implemented (the backward of the message-passing kernels is missing): call under "
                                      "torch.no_grad() or freeze the module")
        require_gpu(x, "V2VNetFusion.forward")
        with torch.no_grad():
            return self._forward_hip(f32c(x), lens, affine_matrix)

    def _round(self, h, theta, src_row, node_row, pair_off, nodes_index):
        """One round for the nodes `node_row` (rows of h): their new states [n_nodes, C, H, W]."""
        l, dev = _lib.lib(), h.device
        st = stream_ptr(dev)
        _, C, H, W = h.shape
        P, n_nodes = theta.shape[0], node_row.shape[0]
        m = self.msg_cnn
        warped = torch.empty(P, C, H, W, dtype=torch.float32, device=dev)
        _lib.check(l.gencomm_v2v_warp_pairs_fwd(ptr(h), ptr(theta), ptr(src_row), ptr(warped), P, C, H, W, st), "gencomm_v2v_warp_pairs_fwd")
        y = self._conv(warped, self._weights("msg_src", [m.weight], lambda: (m.weight[:, :C], None), 3, dev))
        hn = h if nodes_index is None else h.index_select(0, nodes_index)
        e = self._conv(hn, self._weights("msg_node", [m.weight, m.bias], lambda: (m.weight[:, C:], m.bias), 3, dev))
        out = torch.empty(n_nodes, 2 * C if self.gru_flag else C, H, W, dtype=torch.float32, device=dev)
        _lib.check(l.gencomm_v2v_aggregate_fwd(ptr(y), ptr(e), ptr(h), ptr(theta), ptr(node_row), ptr(pair_off), ptr(out), n_nodes, C, H, W,
                                               AGG_OPERATORS.index(self.agg_operator), 0 if self.gru_flag else 1, st), "gencomm_v2v_aggregate_fwd")
        if not self.gru_flag:
            return out
        for layer in range(len(self.kernel_sizes)):
            g = self._conv(out, self._cell_weights(layer, dev))
            out = torch.empty(n_nodes, C, H, W, dtype=torch.float32, device=dev)
            _lib.check(l.gencomm_gru_gate_fwd(ptr(g), ptr(out), n_nodes, C, H * W, st), "gencomm_gru_gate_fwd")
        return out

    def _forward_hip(self, x, lens, affine_matrix):
        dev = x.device
        C = x.shape[1]
        off = [0]
        for k in lens:
            off.append(off[-1] + k)
        ego_rows = off[:-1]
        aff = affine_matrix.to(dev)
        # theta of every pair by slicing (no index lists: normalize_pairwise_tfm says why); pairs are ordered (scene, target i, source j)
        h = x
        if self.num_iteration > 1:
            theta = torch.cat([aff[b, :k, :k].reshape(k * k, 2, 3) for b, k in enumerate(lens)], 0).to(torch.float64).contiguous()
            src_row = dev_ints([off[b] + j for b, k in enumerate(lens) for _ in range(k) for j in range(k)], dev)
            node_row = dev_ints(range(off[-1]), dev)
            po = [0]
            for k in lens:
                po.extend([po[-1] + k * (i + 1) for i in range(k)])
            pair_off = dev_ints(po, dev)
            for _ in range(self.num_iteration - 1):
                h = self._round(h, theta, src_row, node_row, pair_off, None)
        # the last round: only node 0 of every scene is read afterwards (fusion_in_one.py:348-349)
        theta = torch.cat([aff[b, 0, :k] for b, k in enumerate(lens)], 0).to(torch.float64).contiguous()
        src_row = dev_ints(range(off[-1]), dev)
        nodes_index = None if all(k == 1 for k in lens) else dev_ints(ego_rows, dev, torch.int64)
        h = self._round(h, theta, src_row, dev_ints(ego_rows, dev), dev_ints(off, dev), nodes_index)
        lin = self.mlp
        prepared, ss, cin, cout, _ = self._weights("mlp", [lin.weight, lin.bias], lambda: (lin.weight[:, :, None, None], lin.bias), 1, dev)
        from .v2xvit import _linear
        return _linear(h, (prepared, ss, cin, cout))
