"""Generates ``tests/golden/reference_loader.json`` by RUNNING THE REFERENCE's own loader on the INTEGRATION.md stub.

    PYTHONDONTWRITEBYTECODE=1 python tests/make_reference_loader_golden.py <kernel-matrix-benchmarks checkout>

Runs test_reference_binding.py's child (the reference's ``get_definitions`` / ``algorithm_status`` /
``instantiate_algorithm`` on the stub module and ``algos.yaml`` entries of INTEGRATION.md section 1) and stores
its OUTPUT: definition counts, statuses, modules and the plugin instances it built.  Nothing of the reference is stored.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import test_reference_binding as binding  # noqa: E402


def main(reference):
    stub, yaml_text = binding.integration_blocks()
    with tempfile.TemporaryDirectory() as tmp:
        overlay = os.path.join(tmp, "overlay")
        os.makedirs(os.path.join(overlay, "algorithms"))
        with open(os.path.join(overlay, "algorithms", "mi355x.py"), "w") as f:
            f.write(stub)
        with open(os.path.join(overlay, "algos.yaml"), "w") as f:
            f.write(yaml_text)
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        env.pop("PYTHONPATH", None)
        run = subprocess.run([sys.executable, "-c", binding.CHILD, overlay, os.path.abspath(reference), binding.ROOT],
                             capture_output=True, text=True, env=env, cwd=tmp, timeout=300, check=True)
    out = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    with open(os.path.join(HERE, "golden", "reference_loader.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"{len(out['instances'])} instances written")


if __name__ == "__main__":
    main(sys.argv[1])
