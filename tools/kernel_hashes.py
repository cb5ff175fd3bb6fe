"""Per-kernel code hashes of libgrt.so's gfx950 kernels (no GPU needed).

    python tools/kernel_hashes.py [--lib PATH] [--out FILE]

Prints (or writes) {mangled kernel name: _lib.kernel_code_sha256} for every kernel in
namespace grt of the library's code objects.  A change that must leave existing kernels
alone is checked by running this on a build of the parent commit and on a build of the
change: the hashes of the kernels both have must be equal
(profiles/sequence/kernel_hashes.json holds such a pair)."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def kernel_hashes(lib_path):
    from gr_raytracer_amd import _lib

    names = sorted({s for s in _lib.kernel_symbols(lib_path) if s.startswith("_ZN3grt")})
    return {s: _lib.kernel_code_sha256(s, lib_path) for s in names}


if __name__ == "__main__":
    from gr_raytracer_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=str(_lib.LIB_PATH))
    ap.add_argument("--out")
    a = ap.parse_args()
    text = json.dumps(kernel_hashes(Path(a.lib)), indent=1) + "\n"
    if a.out:
        Path(a.out).write_text(text)
    else:
        sys.stdout.write(text)
