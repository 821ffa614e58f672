"""Writes tests/golden/convnext_flow.npz: the reference's own network/image_fe.py::ImageFE('convnext_tiny', '2_1_2') run on
the CPU restatement of the network (tests/convnext_ref.py) with seeded weights.  It pins the truncation and the tap points of
the trunk to the reference's control flow, as glue.npz does for forward_resnet.

    python tests/golden/make_convnext_flow.py <path of the reference checkout>

torchvision is stubbed in sys.modules: models.convnext_tiny(...) returns randomize_convnext(ConvNeXtTiny(), SEED) in fp64.
The fixture holds data only: the input, the three maps, last_dim and the state_dict key list.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import convnext_ref  # noqa: E402

SEED, LAYERS, SHAPE = 20, "2_1_2", (1, 3, 32, 40)


def main(ref_root):
    def convnext_tiny(*args, **kwargs):
        torch.manual_seed(0)
        return convnext_ref.randomize_convnext(convnext_ref.ConvNeXtTiny(), SEED).double().eval()

    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.convnext_tiny = convnext_tiny
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    spec = importlib.util.spec_from_file_location("ref_network_image_fe", os.path.join(ref_root, "network", "image_fe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fe = mod.ImageFE("convnext_tiny", LAYERS).eval()
    x = torch.from_numpy(np.random.default_rng(SEED + 1).standard_normal(SHAPE).astype(np.float32)).double()
    convnext_ref.check_weights_are_felt(fe.fe, x)
    with torch.no_grad():
        last, maps = fe(x)
    assert last is maps[-1] and len(maps) == 3
    np.savez_compressed(os.path.join(HERE, "convnext_flow.npz"), x=x.numpy().astype(np.float32),
                        map0=maps[0].numpy(), map1=maps[1].numpy(), map2=maps[2].numpy(), last_dim=np.int64(fe.last_dim),
                        keys=np.array(list(fe.fe.state_dict().keys())), seed=np.int64(SEED), layers=np.array(LAYERS))


if __name__ == "__main__":
    main(sys.argv[1])
