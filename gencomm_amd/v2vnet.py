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

By default the module infers only: a call with gradients enabled into a module that has a parameter or an input requiring grad raises
``NotImplementedError``. ``V2VNetFusion(args, trainable=True)`` sends such a call through ``autograd.V2VNetFunction`` instead (the
precedent is ``LiftSplatShoot(args, trainable=True)``). Its forward is the forward above with ``gencomm_v2v_aggregate_train_fwd`` (the
same bits, plus the winner map for max) and keeps, per round, the round's input states, ``[h | agg]``, each GRU layer's pre-activation
and input, and the winner map -- not the P warped maps, nor the two halves of the message convolution. Backward, per round in reverse:
  mlp (last round)              1x1 weight gradient and input gradient
  per GRU layer, last first     gencomm_gru_gate_bwd, then train_ops.conv2d_wgrad_fixed / conv2d_dgrad with the stacked weights
  aggregation                   gencomm_v2v_aggregate_bwd -> d y [P], d e [n_nodes]; the gradient of h_k is a slice of d [h | agg]
  source half of msg_cnn        gencomm_v2v_warp_pairs_fwd AGAIN (the warped maps are the weight gradient's input), conv2d_wgrad_fixed, conv2d_dgrad
  node half of msg_cnn          conv2d_wgrad_fixed (with the bias gradient), conv2d_dgrad
  warp                          gencomm_v2v_warp_pairs_bwd, accumulate = 1, into the sum of the two node-side gradients
The ego-only last round hands its gradient to the ego rows; the other rows get zeros from it. The gradients land on the reference's
full-shape parameters: ``msg_cnn.weight.grad = cat[d W_src, d W_node]``, a cell's stacked gradient in ``conv_gates.weight.grad[C:, :cin]``,
``conv_gates.bias.grad[C:]``, ``conv_can.weight.grad[:, :cin]`` and ``conv_can.bias.grad`` -- the reset-gate rows and the hidden-state
columns are exact zeros (tensors, as the reference's autograd yields: they multiply a zero hidden state), and with ``gru_flag: false`` the
``conv_gru`` parameters get no gradient at all. ``affine_matrix`` gets none. Frozen parameters skip their weight gradients; an input that
does not require grad skips the first round's input gradients.
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
def pairs_by_source_row(src_row, rows):
    """The pairs grouped by the row they read, as a CSR: (row_pair_off [rows + 1], row_pairs [P]); the pairs of a row in ascending order."""
    off = [0] * (rows + 1)
    for r in src_row:
        off[r + 1] += 1
    for r in range(rows):
        off[r + 1] += off[r]
    return off, sorted(range(len(src_row)), key=lambda p: (src_row[p], p))


class V2VNetFusion(nn.Module):
    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
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
            if not self.trainable:
                raise NotImplementedError("v2vnet training is not implemented (the backward of the message-passing kernels is missing): call "
                                          "under torch.no_grad() or freeze the module")
            require_gpu(x, "V2VNetFusion.forward")
            from .autograd import V2VNetFunction
            names, params = zip(*self.named_parameters())
            return V2VNetFunction.apply(self, lens, affine_matrix, names, x, *params)
        require_gpu(x, "V2VNetFusion.forward")
        with torch.no_grad():
            return self._forward_hip(f32c(x), lens, affine_matrix)

    def _round(self, h, theta, src_row, node_row, pair_off, nodes_index, keep=None):
        """One round for the nodes `node_row` (rows of h): their new states [n_nodes, C, H, W]. `keep` (a dict, training): the aggregation
        runs through the training entry and the dict receives what the backward reads."""
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
        op = AGG_OPERATORS.index(self.agg_operator)
        if keep is None:
            _lib.check(l.gencomm_v2v_aggregate_fwd(ptr(y), ptr(e), ptr(h), ptr(theta), ptr(node_row), ptr(pair_off), ptr(out), n_nodes, C, H, W,
                                                   op, 0 if self.gru_flag else 1, st), "gencomm_v2v_aggregate_fwd")
        else:
            winner = torch.empty(n_nodes, C, H, W, dtype=torch.uint8, device=dev) if op == 1 else None
            _lib.check(l.gencomm_v2v_aggregate_train_fwd(ptr(y), ptr(e), ptr(h), ptr(theta), ptr(node_row), ptr(pair_off), ptr(out), ptr(winner),
                                                         n_nodes, C, H, W, op, 0 if self.gru_flag else 1, st), "gencomm_v2v_aggregate_train_fwd")
            keep.update(h=h, winner=winner, layers=[])
        if not self.gru_flag:
            return out
        for layer in range(len(self.kernel_sizes)):
            g = self._conv(out, self._cell_weights(layer, dev))
            if keep is not None:
                keep["layers"].append((out, g))           # the layer's input ([h | agg] for the first) and its pre-activation
            out = torch.empty(n_nodes, C, H, W, dtype=torch.float32, device=dev)
            _lib.check(l.gencomm_gru_gate_fwd(ptr(g), ptr(out), n_nodes, C, H * W, st), "gencomm_gru_gate_fwd")
        return out

    def _forward_hip(self, x, lens, affine_matrix, rounds=None):
        """`rounds` (a list, training): one record per round -- the pair tables and what `_round` keeps -- and the states `mlp` reads."""
        dev = x.device
        off = [0]
        for k in lens:
            off.append(off[-1] + k)
        ego_rows = off[:-1]
        aff = affine_matrix.to(dev)
        # theta of every pair by slicing (no index lists: normalize_pairwise_tfm says why); pairs are ordered (scene, target i, source j)
        h = x
        if self.num_iteration > 1:
            theta = torch.cat([aff[b, :k, :k].reshape(k * k, 2, 3) for b, k in enumerate(lens)], 0).to(torch.float64).contiguous()
            src = [off[b] + j for b, k in enumerate(lens) for _ in range(k) for j in range(k)]
            src_row = dev_ints(src, dev)
            node_row = dev_ints(range(off[-1]), dev)
            po = [0]
            for k in lens:
                po.extend([po[-1] + k * (i + 1) for i in range(k)])
            pair_off = dev_ints(po, dev)
            for _ in range(self.num_iteration - 1):
                keep = self._record(rounds, theta, src, src_row, node_row, pair_off, None, off[-1], dev)
                h = self._round(h, theta, src_row, node_row, pair_off, None, keep)
        # the last round: only node 0 of every scene is read afterwards (fusion_in_one.py:348-349)
        theta = torch.cat([aff[b, 0, :k] for b, k in enumerate(lens)], 0).to(torch.float64).contiguous()
        src_row = dev_ints(range(off[-1]), dev)
        nodes_index = None if all(k == 1 for k in lens) else dev_ints(ego_rows, dev, torch.int64)
        keep = self._record(rounds, theta, list(range(off[-1])), src_row, dev_ints(ego_rows, dev), dev_ints(off, dev), nodes_index, off[-1], dev)
        h = self._round(h, theta, src_row, dev_ints(ego_rows, dev), dev_ints(off, dev), nodes_index, keep)
        if rounds is not None:
            rounds.append(h)
        lin = self.mlp
        prepared, ss, cin, cout, _ = self._weights("mlp", [lin.weight, lin.bias], lambda: (lin.weight[:, :, None, None], lin.bias), 1, dev)
        from .v2xvit import _linear
        return _linear(h, (prepared, ss, cin, cout))

    # ---- training (autograd.V2VNetFunction)
    @staticmethod
    def _record(rounds, theta, src, src_row, node_row, pair_off, nodes_index, rows, dev):
        if rounds is None:
            return None
        rpo, rp = pairs_by_source_row(src, rows)
        keep = dict(theta=theta, src_row=src_row, node_row=node_row, pair_off=pair_off, nodes_index=nodes_index,
                    row_pair_off=dev_ints(rpo, dev), row_pairs=dev_ints(rp, dev))
        rounds.append(keep)
        return keep

    def _backward_hip(self, rounds, w, need, need_x, grad_out):
        """`rounds`: what `_forward_hip` recorded; `w`: name -> parameter as the forward saw it; `need`: name -> whether that parameter
        wants a gradient. Returns (d x or None, {name: gradient}) with the gradients in the parameters' full shapes."""
        from . import train_ops as T
        l, dev = _lib.lib(), grad_out.device
        st = stream_ptr(dev)
        C, H, W = self.in_channels, self.H, self.W
        op, out_mode = AGG_OPERATORS.index(self.agg_operator), 0 if self.gru_flag else 1
        *recs, h_last = rounds
        part = {}                                    # sums over the rounds, in the kernels' own shapes

        def add(key, g):
            part[key] = g if key not in part else part[key] + g

        def empty(*shape):
            return torch.empty(*shape, dtype=torch.float32, device=dev)

        if need["mlp.weight"] or need["mlp.bias"]:
            dw, db = T.conv2d_wgrad_fixed(grad_out, h_last, 1, True)
            add("mlp", (dw[:, :, 0, 0], db))
        d = T.conv2d_dgrad(grad_out, w["mlp.weight"][:, :, None, None], 0)
        w_msg = w["msg_cnn.weight"]
        need_msg = need["msg_cnn.weight"] or need["msg_cnn.bias"]
        cells = [f"conv_gru.cell_list.{i}." for i in range(len(self.kernel_sizes))]
        for ri in reversed(range(len(recs))):
            r = recs[ri]
            theta, h = r["theta"], r["h"]
            P, n_nodes, rows = theta.shape[0], r["node_row"].shape[0], h.shape[0]
            need_dh = need_x or ri > 0
            if self.gru_flag:
                for i in reversed(range(len(cells))):
                    inp, g = r["layers"][i]
                    k, cin = self.kernel_sizes[i][0], inp.shape[1]
                    dg = empty(n_nodes, 2 * C, H, W)
                    _lib.check(l.gencomm_gru_gate_bwd(ptr(g), ptr(d), ptr(dg), n_nodes, C, H * W, st), "gencomm_gru_gate_bwd")
                    if any(need[cells[i] + t] for t in ("conv_gates.weight", "conv_gates.bias", "conv_can.weight", "conv_can.bias")):
                        dw, db = T.conv2d_wgrad_fixed(dg, inp, k, True)
                        add(cells[i], torch.cat([dw.reshape(-1), db]))
                    if i > 0 or need_msg or need_dh:
                        stacked = torch.cat([w[cells[i] + "conv_gates.weight"][C:, :cin], w[cells[i] + "conv_can.weight"][:, :cin]], 0)
                        d = T.conv2d_dgrad(dg, stacked, k // 2)
            if not (need_msg or need_dh):
                break
            dy, de = empty(P, C, H, W), empty(n_nodes, C, H, W)     # d is now d [h | agg] (GRU) or d (h + agg)
            _lib.check(l.gencomm_v2v_aggregate_bwd(ptr(d), ptr(theta), ptr(r["node_row"]), ptr(r["pair_off"]), ptr(r["winner"]), ptr(dy), ptr(de),
                                                   n_nodes, C, H, W, op, out_mode, st), "gencomm_v2v_aggregate_bwd")
            if need_msg:
                warped = empty(P, C, H, W)           # recomputed, not kept: one gather against P maps held per round
                _lib.check(l.gencomm_v2v_warp_pairs_fwd(ptr(h), ptr(theta), ptr(r["src_row"]), ptr(warped), P, C, H, W, st), "gencomm_v2v_warp_pairs_fwd")
                dws, _ = T.conv2d_wgrad_fixed(dy, warped, 3, False)
                del warped
                hn = h if r["nodes_index"] is None else h.index_select(0, r["nodes_index"])
                dwn, db = T.conv2d_wgrad_fixed(de, hn, 3, True)
                add("msg", torch.cat([dws.reshape(-1), dwn.reshape(-1), db]))
            if not need_dh:
                break
            dwarped = T.conv2d_dgrad(dy, w_msg[:, :C], 1)
            del dy
            dn = T.conv2d_dgrad(de, w_msg[:, C:], 1)
            dn += d[:, :C] if self.gru_flag else d   # the pass-through gradient of h_k
            if r["nodes_index"] is None:
                dh = dn
            else:                                    # the ego-only round: the other rows get nothing from it but what the warp brings
                dh = torch.zeros(rows, C, H, W, dtype=torch.float32, device=dev)
                dh.index_copy_(0, r["nodes_index"], dn)
            scratch = empty(_lib.check_size(l.gencomm_v2v_warp_pairs_bwd_scratch_floats(P), "gencomm_v2v_warp_pairs_bwd_scratch_floats"))
            _lib.check(l.gencomm_v2v_warp_pairs_bwd(ptr(dwarped), ptr(theta), ptr(r["src_row"]), ptr(r["row_pair_off"]), ptr(r["row_pairs"]), ptr(dh),
                                                    ptr(scratch), P, rows, C, H, W, 1, st), "gencomm_v2v_warp_pairs_bwd")
            d = dh
        # ---- onto the reference's full-shape parameters
        grads = {}
        if "mlp" in part:
            grads["mlp.weight"], grads["mlp.bias"] = part["mlp"]
        if "msg" in part:
            nw = C * C * 9
            grads["msg_cnn.weight"] = torch.cat([part["msg"][:nw].view(C, C, 3, 3), part["msg"][nw:2 * nw].view(C, C, 3, 3)], 1)
            grads["msg_cnn.bias"] = part["msg"][2 * nw:]
        for i, pre in enumerate(cells):
            if pre not in part:
                continue
            k = self.kernel_sizes[i][0]
            cin = self.conv_gru.cell_list[i].input_dim
            dw, db = part[pre][:2 * C * cin * k * k].view(2 * C, cin, k, k), part[pre][2 * C * cin * k * k:]
            gw, cw = torch.zeros_like(w[pre + "conv_gates.weight"]), torch.zeros_like(w[pre + "conv_can.weight"])
            gb = torch.zeros_like(w[pre + "conv_gates.bias"])
            gw[C:, :cin], cw[:, :cin], gb[C:] = dw[:C], dw[C:], db[:C]   # reset-gate rows and hidden-state columns: exact zeros
            grads.update({pre + "conv_gates.weight": gw, pre + "conv_gates.bias": gb, pre + "conv_can.weight": cw, pre + "conv_can.bias": db[C:]})
        return (d if need_x else None), {k: v for k, v in grads.items() if need[k]}
