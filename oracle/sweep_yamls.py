#!/usr/bin/env python3
"""Constructs this build's model shell from EVERY yaml the reference ships under ``opencood/hypes_yaml/**/GenComm_yamls/**``
(VERDICT r2 item 9 i: the hypes_yaml config surface swept, not asserted) and records, per yaml, either
``{"core_method", "keys", "hash"}`` -- the number of checkpoint keys and a hash of the sorted (key, shape) pairs of the
constructed module's ``state_dict`` -- or the reason it cannot be built (``NotImplementedError`` text naming the yaml key, or
"not a GenComm model" for the baseline methods' yamls, whose ``core_method`` this build does not provide).

Run where /root/reference is mounted (CPU only; test infrastructure like the rest of oracle/):

    python oracle/sweep_yamls.py            # writes tests/golden/yaml_sweep.json and tests/golden/yaml_sweep_models.json.gz

The yamls themselves are not committed: the report and, as the sweep's input fixture, the ``model`` block of every yaml as
parsed (``yaml_sweep_models.json.gz``, gzip-compressed JSON), so that ``tests/test_yaml_sweep.py`` re-runs the sweep without the reference. Loading mirrors ``opencood/hypes_yaml/yaml_utils.py:14-49`` as far as the model
block needs it: PyYAML with the float resolver the reference adds (:22-35); the ``yaml_parser`` post-parsers
(``load_general_params`` :337-370 ...) only add anchor geometry under ``postprocess`` / ``preprocess``, which the model
constructor does not read."""
import glob
import gzip
import hashlib
import importlib
import json
import os
import re
import sys

import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REF_YAMLS = "/root/reference/opencood/hypes_yaml"
OUT = os.path.join(REPO, "tests", "golden", "yaml_sweep.json")
MODELS = os.path.join(REPO, "tests", "golden", "yaml_sweep_models.json.gz")


def load_yaml(path):
    loader = yaml.Loader
    loader.add_implicit_resolver(   # the float forms PyYAML's default resolver misses (1e-3, .5e2, ...): yaml_utils.py:22-35
        u'tag:yaml.org,2002:float',
        re.compile(u'''^(?:
         [-+]?(?:[0-9][0-9_]*)\\.[0-9_]*(?:[eE][-+]?[0-9]+)?
        |[-+]?(?:[0-9][0-9_]*)(?:[eE][-+]?[0-9]+)
        |\\.[0-9_]+(?:[eE][-+][0-9]+)?
        |[-+]?[0-9][0-9_]*(?::[0-5]?[0-9])+\\.[0-9_]*
        |[-+]?\\.(?:inf|Inf|INF)
        |\\.(?:nan|NaN|NAN))$''', re.X),
        list(u'-+0123456789.'))
    with open(path) as f:
        return yaml.load(f, Loader=loader)


def resolve(core_method):
    """opencood/tools/train_utils.py:269-287 with the package prefix swapped: module by file name, class by lower-cased name."""
    try:
        lib = importlib.import_module("gencomm_amd." + core_method)
    except ImportError:
        return None
    target = core_method.replace("_", "").lower()
    for name, cls in lib.__dict__.items():
        if name.lower() == target:
            return cls
    return None


def read_models():
    """{yaml path relative to hypes_yaml: its ``model`` block as parsed} for every GenComm_yamls yaml of the reference."""
    models = {}
    for path in sorted(glob.glob(os.path.join(REF_YAMLS, "**", "GenComm_yamls", "**", "*.yaml"), recursive=True)):
        hypes = load_yaml(path)
        models[os.path.relpath(path, REF_YAMLS)] = hypes.get("model") if isinstance(hypes, dict) else None
    return models


def load_models():
    """The committed fixture of :func:`read_models`."""
    with gzip.open(MODELS, "rt") as f:
        return json.load(f)


def sweep(models):
    report = {}
    for name, model in models.items():
        try:
            core = model["core_method"]
            cls = resolve(core)
            if cls is None:
                report[name] = {"core_method": core, "built": False, "reason": "not a GenComm model: core_method is a baseline method's shell"}
                continue
            built = cls(model["args"])
            pairs = sorted((k, list(v.shape)) for k, v in built.state_dict().items())
            h = hashlib.sha256(json.dumps(pairs).encode()).hexdigest()[:16]
            report[name] = {"core_method": core, "built": True, "keys": len(pairs), "hash": h,
                            "params": int(sum(p.numel() for p in built.parameters()))}
        except NotImplementedError as e:
            report[name] = {"core_method": model["core_method"], "built": False, "reason": "NotImplementedError: " + str(e)}
        except Exception as e:  # anything else is a defect of the build or of the yaml: recorded verbatim
            report[name] = {"core_method": model.get("core_method") if isinstance(model, dict) else None,
                            "built": False, "reason": f"{type(e).__name__}: {e}"}
    return report


if __name__ == "__main__":
    if not os.path.isdir(REF_YAMLS):
        raise SystemExit("the reference checkout is not mounted: nothing to sweep")
    models = read_models()
    with open(MODELS, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as gz:   # mtime 0: the same yamls give the same bytes
        gz.write(json.dumps(models, sort_keys=True).encode())
    rep = sweep(models)
    with open(OUT, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
    built = sum(1 for v in rep.values() if v["built"])
    print(f"{len(rep)} yamls: {built} shells built")
    reasons = {}
    for v in rep.values():
        if not v["built"]:
            reasons[v["reason"][:110]] = reasons.get(v["reason"][:110], 0) + 1
    for r, c in sorted(reasons.items(), key=lambda kv: -kv[1]):
        print(f"  {c:3d} x {r}")
