"""Generates tests/golden/pc_rotation.npz from the REFERENCE's own PCRandomRotation._M (pc_augmentation.py:100-101, scipy's
matrix exponential) at three fixed angles about z.  Data only: the angles and the reference's fp32 matrices.

Needs /root/reference and scipy:
    python tests/golden/make_pc_rotation.py
The reference module imports torchvision at import time, which is not installed here: an inert stub stands in for it.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
ANGLES_DEG = (5.0, -3.25, 0.5)


def main():
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    sys.path.insert(0, REF)
    import pc_augmentation
    rot = pc_augmentation.PCRandomRotation(max_theta=5, max_theta2=0, axis=np.array([0, 0, 1]))
    theta = np.array([np.pi * a / 180.0 for a in ANGLES_DEG], dtype=np.float64)
    mats = np.stack([rot._M(rot.axis, t) for t in theta])
    assert mats.dtype == np.float32 and mats.shape == (3, 3, 3)
    np.savez(os.path.join(HERE, "pc_rotation.npz"), theta=theta, matrix=mats)
    print("pc_rotation.npz:", mats.shape)


if __name__ == "__main__":
    main()
