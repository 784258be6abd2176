"""The README's "Environment knobs" table lists exactly the RTDC_* variables the tree reads."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ray_torch_distributed_checkpoint_amd")
LITERAL = re.compile(r'"(RTDC_[A-Z0-9_]+)"')


def _files():
    for top, exts in ((PKG, (".py", ".cpp", ".hip", ".h")), (os.path.join(ROOT, "benchmarks"), None),
                      (os.path.join(ROOT, "scripts"), None)):
        for d, dirs, names in os.walk(top):
            dirs[:] = [x for x in dirs if x not in ("build", "__pycache__")]
            for n in names:
                if exts is None or n.endswith(exts):
                    yield os.path.join(d, n)
    for n in ("bench.py", "train_flow.py", "eval_flow.py"):
        yield os.path.join(ROOT, n)


def _knobs_read():
    found = set()
    for path in _files():
        with open(path, "rb") as f:
            found.update(LITERAL.findall(f.read().decode("utf-8", "replace")))
    return found


def _knobs_documented():
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as f:
        text = f.read()
    table = text.split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    names = set()
    for line in table.splitlines():
        if line.startswith("|"):
            names.update(re.findall(r"`(RTDC_[A-Z0-9_]+)`", line.split("|")[1]))
    return names


def test_readme_knob_table_matches_the_tree():
    read, documented = _knobs_read(), _knobs_documented()
    assert read and documented
    undocumented, stale = sorted(read - documented), sorted(documented - read)
    assert not undocumented and not stale, (
        f"read by the tree but not in README's knob table: {undocumented}; "
        f"in the table but read nowhere: {stale}")
