"""Generate the DCTE_LQR_ALPHA golden maps (run where oracle/_ref was built).

The input is the committed RGBA frame inputs/rgba_45x38.npy.  Its luma plane
is the alpha rule of include/dctenergy.h [liblqr, unverified] -- the RGB
brightness times alpha / 255 in double (tests/alpha_util.py alpha_plane) --
and the expected maps come from the REFERENCE's own transforms over that
plane (oracle/_ref, ref_energy_map_luma), as make_golden.py's do.

Data only: .npy arrays and manifest_alpha.json.

    python tests/golden/make_golden_alpha.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_py as O  # noqa: E402
from alpha_util import NS, WEIGHTS, alpha_plane  # noqa: E402

INPUT = "rgba_45x38.npy"


def main():
    if not O.ref_available():
        raise SystemExit("oracle/_ref is not built (make -C oracle ref)")
    img = np.load(os.path.join(HERE, "inputs", INPUT), allow_pickle=False)
    plane = alpha_plane(img)
    manifest = {
        "generator": "tests/golden/make_golden_alpha.py",
        "expected_outputs": "oracle/_ref (reference src/fft2d transforms, unmodified) over the alpha-weighted plane",
        "luma": "DCTE_LQR_ALPHA: (0.2126*(R/255.) + 0.7152*(G/255.) + 0.0722*(B/255.)) * (A/255.) "
                "(double, that association) [liblqr, unverified]",
        "maps": [],
    }
    for n in NS:
        for e, t in WEIGHTS:
            ofile = f"alpha__rgba_45x38__n{n}_e{e}_t{t}.npy"
            np.save(os.path.join(HERE, "maps", ofile), O.ref_energy_map_luma(plane, n, e, t))
            manifest["maps"].append({"input": INPUT, "output": ofile, "N": n, "edges": e,
                                     "textures": t, "shape": list(img.shape)})
    with open(os.path.join(HERE, "manifest_alpha.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(len(manifest["maps"]), "alpha maps")


if __name__ == "__main__":
    main()
