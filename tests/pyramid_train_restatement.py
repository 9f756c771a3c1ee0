"""One training step of HEAL's PyramidFusion in framework operators, the cases of tests/golden/pyramid_train_*.npz and the error bar of
the pyramid training tests. Shared by tests/test_pyramid_train.py, tests/test_gpu_pyramid_train.py, tools/make_golden_pyramid_train.py
and tools/bench_pyramid_train.py. Nothing here touches the HIP library; ``run_case`` drives any module with PyramidFusion's interface
(the reference's, the restatement, the HIP module)."""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F  # noqa: F401

import pyramid_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILE_LIMIT = 880 * 1024           # bytes per fixture file: no larger than pyramid.npz, the largest pyramid fixture before
SAMPLE_ABOVE = 4096               # a float64 gradient with more elements is stored as a fixed-stride sample + sum + L2 norm
SAMPLES = 2048
H0, W0, C0 = 24, 40, 64           # level 0: divisible by 4, crosses the 8 x 32 tile both ways
RECORD_LEN = [1, 4]
MODALITIES = ["m1", "m1", "m2", "m4", "m1"]      # the camera agents are the two generic (non-ego) agents of scene 1
CROP_INFO = {"m2": {"crop_ratio_W_m2": 2, "crop_ratio_H_m2": 2}, "m4": {"crop_ratio_W_m4": 1, "crop_ratio_H_m4": 1}}
CASES = {
    # name: (mode, frozen parameters, forward)
    "train": ("train", False, "collab"),       # cam_crop_info is passed and ignored, as the reference ignores it when self.training
    "frozen": ("eval", True, "collab"),        # HEAL's new-agent stage: gradients THROUGH a frozen pyramid, crop mask on
    "single": ("train", False, "single"),
}


class PyramidTrainRestatement(R.PyramidRestatement):
    def forward_collab(self, x, record_len, affine, modalities=None, crop=None, levels=None):
        return super().forward_collab(x, record_len, affine, modalities, None if self.training else crop, levels)


def case_inputs(name, record_len=None, hw=None):
    """(x [n, C0, H, W] float32, record_len, affine [B, 5, 5, 2, 3] float64, cotangent of the fused feature, cotangents of the occ maps).
    The cotangents are random and POSITIVE (1/16 + |normal|, on a 1/16 grid). The step has scalars that are judged by their relative
    error: the loss and the three head biases' gradients. With signed cotangents each is what is left of many cancelling terms, and
    its relative error is noise over an accidental remainder: torch's own float32 error of the loss -- half of the bar -- varied by 4x
    between two float32 implementations of the same step. With positive cotangents the loss is dominated by a sum of non-negative terms
    (the fused feature is a ReLU output) and a bias gradient by the sum of its occ cotangent; the tensors are compared element by
    element either way."""
    mode, frozen, fwd = CASES[name]
    rl = list(RECORD_LEN if record_len is None else record_len)
    H, W = (H0, W0) if hw is None else hw
    n = 1 if fwd == "single" else sum(rl)
    seed = R.SEED + 100 + 10 * sorted(CASES).index(name) + (0 if hw is None else 1000 + H)
    x = R.quantised(seed, (n, C0, H, W))
    scenes = R.collab_scenes(H, W)
    if record_len is not None:                  # shorter scenes: each keeps its first poses
        scenes = [s[:k] for s, k in zip(scenes, rl)]
    aff = R.affine_of(scenes, L=5)
    B = 1 if fwd == "single" else len(rl)
    g_f = np.abs(R.quantised(seed + 1, (B, 384, H, W), step=16)) + np.float32(1 / 16)
    g_occ = [np.abs(R.quantised(seed + 2 + i, (n, 1, H >> i, W >> i), step=16)) + np.float32(1 / 16) for i in range(3)]
    return x, rl, aff, g_f, g_occ


def run_case(model, name, dtype, device="cpu", record_len=None, hw=None):
    """One step of case `name` on `model` (already holding its parameters): {'loss', 'dx', 'grads': {key: tensor}, 'stats': {key: tensor},
    'scores': the scores handed to the fuse (collab only, for the margin rule)}."""
    mode, frozen, fwd = CASES[name]
    x, rl, aff, g_f, g_occ = case_inputs(name, record_len, hw)
    model.train(mode == "train")
    for p in model.parameters():
        p.requires_grad_(not frozen)
        p.grad = None
    xt = torch.from_numpy(x).to(device=device, dtype=dtype).requires_grad_(True)
    if fwd == "single":
        fused, occs = model.forward_single(xt)
    else:
        fused, occs = model.forward_collab(xt, torch.tensor(rl), torch.from_numpy(aff), MODALITIES if record_len is None else None,
                                           CROP_INFO if record_len is None else None)
    loss = (fused * torch.from_numpy(g_f).to(fused)).sum()
    for o, g in zip(occs, g_occ):
        loss = loss + (o * torch.from_numpy(g).to(o)).sum()
    loss.backward()
    grads = {k: p.grad.detach() for k, p in model.named_parameters() if p.grad is not None}
    stats = {k: v.detach().clone() for k, v in model.state_dict().items() if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked")}
    return {"loss": loss.detach(), "dx": xt.grad.detach(), "grads": grads, "stats": stats, "occs": [o.detach() for o in occs],
            "fused": fused.detach()}


def level_scores(model, name):
    """The float64 scores of every level as case `name` hands them to the fuse (restatement only): the margin rule's input."""
    mode, frozen, fwd = CASES[name]
    x, rl, aff, _, _ = case_inputs(name)
    model.train(mode == "train")
    levels = []
    with torch.no_grad():
        model.forward_collab(torch.from_numpy(x).to(next(model.parameters()).dtype), torch.tensor(rl), torch.from_numpy(aff), MODALITIES, CROP_INFO, levels)
    return [s for _, s, _ in levels], rl, aff


def restatement(dtype=torch.float64, resnext=True, device="cpu"):
    torch.manual_seed(0)
    return R.fill_params_(PyramidTrainRestatement(R.cfg(resnext=resnext)).to(device=device, dtype=dtype))


class relu_margin:
    """``with relu_margin() as m: <a float64 step of the restatement>``: m.worst = the smallest |input| / rms(input) over every ReLU of the
    step. A step one of whose ReLU inputs lies within float32 rounding of zero has no float32 answer to be compared with: which side
    the element falls on is decided by rounding, and through batch statistics one flipped element moves every gradient below it. A
    case whose inputs a test chooses itself must keep its float64 step away from that (``KINK_MARGIN``); the three fixture cases are
    the issue's and are taken as they come (the reference's own float32 step crosses one of them in ``train``)."""

    def __enter__(self):
        import torch.nn.functional as F
        self.worst, self._F, self._orig = float("inf"), F, F.relu

        def relu(x, inplace=False):
            self.worst = min(self.worst, float(x.detach().abs().min() / x.detach().pow(2).mean().sqrt()))
            return self._orig(x, inplace)

        F.relu = relu
        return self

    def __exit__(self, *exc):
        self._F.relu = self._orig
        return False


KINK_MARGIN = 4e-6     # relative to the layer's rms: an order of magnitude above float32 rounding of a sum of a few hundred terms
# the steps without a fixture (cases of "train"), chosen among small maps as the first that stay clear of every ReLU kink in float64
SMALL = dict(record_len=[1, 3], hw=(8, 12))     # resnext false: a lone agent; identity ego + two generic agents
EGO = dict(record_len=[1, 1], hw=(4, 8))        # an ego-only batch: the gradient flows through p_0 = 1


# ------------------------------------------------------------------------------------------- the error bar
def rel_rms(got, ref, floor=0.0):
    """rms(got - ref) / max(rms(ref), floor), in float64."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((got - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), floor, 1e-300))


def bar(e_ref):
    """The project's bar: twice the error of torch's float32 computation of the same thing (the margin is for the summation order),
    and never below 1e-6."""
    return max(2.0 * float(e_ref), 1e-6)


def np64(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


# ------------------------------------------------------------------------------------------- the fixture's storage
def summarise(store, key, ref64):
    """Small tensors whole; large ones as a fixed-stride sample with the float64 sum and L2 norm."""
    a = np64(ref64)
    if a.size <= SAMPLE_ABOVE:
        store[key] = a
        return
    stride = a.size // SAMPLES
    store[key + "#sample"] = a.reshape(-1)[::stride][:SAMPLES].copy()
    store[key + "#meta"] = np.array([a.size, stride, a.sum(), np.sqrt((a ** 2).sum())], np.float64)


def check_summary(store, key, got64, tol=1e-10):
    """Worst relative deviation of `got64` from what `summarise` stored under `key` (sample: relative to the tensor's rms)."""
    a = np64(got64)
    if key in store:
        ref = store[key]
        assert ref.shape == a.shape, key
        return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)) if ref.size else 0.0
    size, stride, total, norm = store[key + "#meta"]
    assert int(size) == a.size and int(stride) == a.size // SAMPLES, key
    rms = norm / np.sqrt(size)
    s = a.reshape(-1)[::int(stride)][:SAMPLES]
    return float(max(np.abs(s - store[key + "#sample"]).max() / rms, abs(a.sum() - total) / (norm * np.sqrt(size)), abs(np.sqrt((a ** 2).sum()) - norm) / norm))


def save_sharded(prefix, store):
    """Write `store` as prefix_0.npz, prefix_1.npz ...: arrays too large for one file are split along their first axis (key@i)."""
    for old in glob.glob(prefix + "_*.npz"):
        os.remove(old)
    pieces = []
    for k, v in store.items():
        v = np.asarray(v)
        if v.nbytes <= FILE_LIMIT * 3 // 4:
            pieces.append((k, v))
        else:
            rows = max(1, (FILE_LIMIT * 3 // 4) // (v.nbytes // v.shape[0]))      # whole rows of the first axis per piece
            pieces.extend((f"{k}@{i}", v[r:r + rows]) for i, r in enumerate(range(0, v.shape[0], rows)))
    files, cur, size = [], {}, 0
    for k, v in sorted(pieces, key=lambda kv: -kv[1].nbytes):
        if cur and size + v.nbytes > FILE_LIMIT * 3 // 4:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    files.append(cur)
    paths = []
    for i, f in enumerate(files):
        paths.append(f"{prefix}_{i}.npz")
        np.savez_compressed(paths[-1], **f)
        assert os.path.getsize(paths[-1]) <= FILE_LIMIT, (paths[-1], os.path.getsize(paths[-1]))
    return paths


def load_sharded(prefix):
    raw = {}
    paths = sorted(glob.glob(prefix + "_*.npz"))
    assert paths, prefix
    for p in paths:
        with np.load(p) as z:
            raw.update({k: z[k] for k in z.files})
    out, split = {}, {}
    for k, v in raw.items():
        if "@" in k:
            base, i = k.rsplit("@", 1)
            split.setdefault(base, {})[int(i)] = v
        else:
            out[k] = v
    for base, parts in split.items():
        out[base] = np.concatenate([parts[i] for i in range(len(parts))], axis=0)
    return out, paths


def fixture(name):
    return load_sharded(os.path.join(GOLDEN, f"pyramid_train_{name}"))
