"""Which kernel instantiations do the guard-band tests dispatch?  A report, not a test (needs an MI355X).

    python tools/guard_dispatch_ids.py [--write]

runs tests/test_conv_guard_gpu.py, test_wgrad_guard_gpu.py and test_pack_guard_gpu.py, then the cases with h <= 72 of
tests/test_kernels_gpu.py, test_x3_gpu.py and test_bf16_gpu.py, each in a child pytest process with this file loaded as a plugin: the
library's launch profiler (ctl_prof_start / ctl_prof_stop, one id per kernel instantiation family) brackets every test.  Prints the ids of
the second set that the first does not reach, with the tests that reach them; --write regenerates profiles/guard_dispatch_ids.txt."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARDED = ["tests/test_conv_guard_gpu.py", "tests/test_wgrad_guard_gpu.py", "tests/test_pack_guard_gpu.py"]
EXISTING = ["tests/test_kernels_gpu.py", "tests/test_x3_gpu.py", "tests/test_bf16_gpu.py"]
MAX_H = 72
IDS = {}


# ------------------------------------------------------------------------------------------------ the plugin side (child processes)
def pytest_collection_modifyitems(config, items):
    max_h = int(os.environ.get("GUARD_IDS_MAX_H", "0"))
    if not max_h:
        return
    keep, drop = [], []
    for it in items:
        cs = getattr(it, "callspec", None)
        h = cs.params.get("h") if cs else None
        (drop if isinstance(h, int) and h > max_h else keep).append(it)
    if drop:
        config.hook.pytest_deselected(items=drop)
        items[:] = keep


def pytest_runtest_setup(item):
    from cooperative_training_and_latent_space_data_augmentation_amd import _ffi
    _ffi.prof_start("")


def pytest_runtest_teardown(item):
    from cooperative_training_and_latent_space_data_augmentation_amd import _ffi
    IDS[item.nodeid] = sorted(_ffi.prof_stop())


def pytest_sessionfinish(session):
    out = os.environ.get("GUARD_IDS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(IDS, f)


# ------------------------------------------------------------------------------------------------ the report
def collect(files, max_h=0):
    with tempfile.NamedTemporaryFile(suffix=".json", delete=False) as t:
        path = t.name
    env = dict(os.environ, GUARD_IDS_OUT=path, GUARD_IDS_MAX_H=str(max_h), PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tools"), ROOT, os.environ.get("PYTHONPATH", "")]))
    rc = subprocess.run([sys.executable, "-m", "pytest", *files, "-m", "gpu", "-q", "-p", "guard_dispatch_ids", "-p", "no:cacheprovider"], cwd=ROOT, env=env).returncode
    with open(path) as f:
        ids = json.load(f)
    os.unlink(path)
    if rc != 0:
        raise SystemExit(f"pytest {' '.join(files)} ended with {rc}")
    return ids


def main():
    guarded, existing = collect(GUARDED), collect(EXISTING, MAX_H)
    got = sorted({i for v in guarded.values() for i in v})
    missing = {}
    for test, ids in existing.items():
        for i in ids:
            if i not in got:
                missing.setdefault(i, []).append(test)
    print(f"{len(got)} ids dispatched by the guard-band tests; {len({i for v in existing.values() for i in v})} by the existing cases with h <= {MAX_H}; "
          f"{len(missing)} of those not reached:")
    for i in sorted(missing):
        print(f"  {i}  <- {', '.join(missing[i][:2])}")
    if "--write" in sys.argv:
        with open(os.path.join(ROOT, "profiles", "guard_dispatch_ids.txt"), "w") as f:
            f.write(f"# python tools/guard_dispatch_ids.py --write: {len(got)} kernel instantiation ids dispatched by {', '.join(GUARDED)}\n")
            f.write(f"# ids reached by the cases with h <= {MAX_H} of {', '.join(EXISTING)} and not by these: {len(missing)}\n")
            for i in sorted(missing):
                f.write(f"#   {i}  <- {missing[i][0]}\n")
            f.write("\n".join(got) + "\n")


if __name__ == "__main__":
    main()
