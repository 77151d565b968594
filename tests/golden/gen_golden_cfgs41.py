"""Drop-in check data for the ablation table: the flat experiment dicts the reference's own generator emits for experiment 41
(`experiments.generate_experiment_cfgs(41)`: six rows on two label splits), keyed by their experiment name.  Data only (JSON), like
gen_golden_cfgs.py, whose file stays as it is.  Runs only where the reference tree exists.  Writes
tests/golden/experiment41_cfgs.json."""
import contextlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def main():
    os.chdir(REF)
    sys.path.insert(0, REF)
    import experiments
    with contextlib.redirect_stderr(io.StringIO()):
        cfgs = experiments.generate_experiment_cfgs(41)
    out = {}
    for c in cfgs:
        assert c["name"] not in out, c["name"]
        out[c["name"]] = c
    path = os.path.join(HERE, "experiment41_cfgs.json")
    json.dump(out, open(path, "w"), indent=1, sort_keys=True, default=lambda o: list(o))
    print("wrote", path, os.path.getsize(path), "bytes", len(out), "rows")


if __name__ == "__main__":
    main()
