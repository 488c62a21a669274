"""Record the package layout of a 3DTopia-XL checkout - file names only, no file contents:

    python tests/golden/make_reference_layout.py /path/to/3DTopia-XL

Writes tests/golden/reference_layout.json: the relative path of every .py file under the checkout's top-level packages
`models/`, `dva/` and `utils/` (which directories carry an __init__.py and which are namespace directories follows from
the list).  tests/test_compat_shim.py::test_against_the_real_reference_layout rebuilds that tree from stub modules, so the
drop-in shim is checked against the real layout without the checkout itself.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PACKAGES = ("models", "dva", "utils")


def main(root: str) -> None:
    files = []
    for pkg in PACKAGES:
        for d, _, names in os.walk(os.path.join(root, pkg)):
            files += [os.path.relpath(os.path.join(d, n), root).replace(os.sep, "/") for n in names if n.endswith(".py")]
    out = {"what": "relative paths of the .py files of a 3DTopia-XL checkout's models/, dva/ and utils/ (names only)",
           "packages": list(PACKAGES), "files": sorted(files)}
    with open(os.path.join(HERE, "reference_layout.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
