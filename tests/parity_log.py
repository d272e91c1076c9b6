"""Driver-visible record of what the GPU parity tests measured (pytest -q drops their prints): per test max / mean |err|,
max |dlogp|, flipped frames and the largest reference margin among them.  Written at session end to
$PAFC_PARITY_DIR/parity_r06.json -- a run on a remote GPU machine points PAFC_PARITY_DIR at the directory its outputs are
collected from -- by default to the git-ignored build/parity_r06.json, so that a test run leaves the tracked tree as it was
(the record committed under profiles/ is refreshed by copying this file there by hand); entries of earlier (partial) runs
are kept, same-named ones replaced."""
import json
import os
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REC = {}


def record(name: str, **values):
    ent = _REC.setdefault(name, {})
    for k, v in values.items():
        ent[k] = (round(float(v), 9) if isinstance(v, float) or hasattr(v, "item") else v)


def flush():
    if not _REC:
        return
    import torch
    meta = {"written": time.strftime("%Y-%m-%d %H:%M:%S"),
            "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "cpu"}
    path = os.path.join(os.environ.get("PAFC_PARITY_DIR") or os.path.join(ROOT, "build"), "parity_r06.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        try:
            with open(path) as f:
                doc = json.load(f)
        except (OSError, ValueError):
            doc = {"tests": {}}
        doc["meta"] = meta
        doc["tests"].update(_REC)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    except OSError:
        pass
