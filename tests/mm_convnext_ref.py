"""fp64 CPU reference of MM.forward_q on the ConvNeXt-tiny trunk (test infrastructure).

The glue of oracle.nets.mm_forward_q (oracle/nets.py:145-218) restated with the three image maps taken from
convnext_ref.forward_maps instead of the oracle's ResNet; everything else is the oracle's own functions (nets.gem,
nets.fuse_block_toshallow, nets.stage2_fuse_block_add, ode.*, oracle.sparse.*).  tests/test_mm_convnext_host.py pins the
restated glue to the oracle: fed the ResNet maps of a resnet18 run it returns the oracle's seven outputs exactly.
"""
import torch
import torch.nn.functional as F

import convnext_ref
from oracle import nets


def options(layers="1_1_1", vox_planes="64_128_384", **kw):
    """The supported configuration of MM with mm_imgfe='convnext_tiny'."""
    from agplace_amd.options import Options
    return Options(mm_imgfe="convnext_tiny", mm_imgfe_layers=layers, mm_imgfe_planes="96_192_384", mm_imgfe_dim=384,
                   mm_stg2fuse_dim=384, mm_voxfe_planes=vox_planes, mm_voxfe_dim=384, **kw)


def seeded_params(opt, seed=0, dtype=torch.float64):
    """(params, trunk): the reference's state_dict of this MM -- fusion and voxel parameters from nets.init_mm_params (called with
    a ResNet in place of the trunk, whose image_fe.fe.* keys are dropped), trunk weights from convnext_ref.seeded_trunk under
    image_fe.fe.* -- and the fp64 trunk itself."""
    p = nets.init_mm_params(opt.copy(mm_imgfe="resnet18"), seed=seed, dtype=dtype)
    p = {k: v for k, v in p.items() if not k.startswith("image_fe.fe.")}
    trunk = convnext_ref.seeded_trunk([int(e) for e in opt.mm_imgfe_layers.split("_")], seed + 11, dtype=dtype)
    p.update({"image_fe.fe." + k: v.detach().clone() for k, v in trunk.state_dict().items()})
    return p, trunk


def forward_q(data_dict, params, opt, trunk=None, maps=None, drop=None):
    """The seven outputs of MM.forward_q.  maps: the image maps (else convnext_ref.forward_maps(trunk, image));
    drop: 'image' / 'pc' as reference mm.py:70-75 (the image, or the cloud's xyz, times zero)."""
    image = data_dict["query_image"]
    if drop == "image":
        image = image * 0
    if drop == "pc":
        data_dict = dict(data_dict)
        c = data_dict["coords"].clone()
        c[:, 1:] = c[:, 1:] * 0
        data_dict["coords"] = c
    if maps is None:
        with torch.no_grad():
            maps = convnext_ref.forward_maps(trunk, image)
    output = []
    imagefeatmap = maps[-1]
    imagefeatvec = nets.gem(imagefeatmap, params["image_pool.p"]).flatten(1)
    if opt.output_l2:
        imagefeatvec = F.normalize(imagefeatvec, dim=-1)
    imagefeatvec_org = imagefeatvec
    output.append(imagefeatvec * params["image_weight"])

    voxmap = None
    if "coords" in data_dict:
        from oracle import sparse
        sp = sparse.from_coords(data_dict["features"].to(image.dtype), data_dict["coords"], nbatch=image.shape[0])
        voxmap, voxmaplist = sparse.minkfpn(sp, params, "vox_fe.", nlevels=len(opt.mm_voxfe_planes.split("_")),
                                            training=False, pattern=None, num_top_down=getattr(opt, "mm_voxfe_ntd", 0))
        data_dict = dict(data_dict)
        data_dict["voxfeatvec"] = sparse.mink_gem(voxmap, params["vox_pool.p"])
        data_dict["vox_levels"] = [sparse.global_avg(e) for e in voxmaplist]
        data_dict["stg2voxvec"] = data_dict["voxvec_fuse"] = None
    voxfeatvec = data_dict["voxfeatvec"]
    if opt.output_l2:
        voxfeatvec = F.normalize(voxfeatvec, dim=-1)
    voxfeatvec_org = voxfeatvec
    output.append(voxfeatvec * params["vox_weight"])

    shallowfeatvec = nets.fuse_block_toshallow(maps, data_dict["vox_levels"], params, "fuseblocktoshallow.", opt)
    shallowfeatvecorg = shallowfeatvec
    if opt.output_l2:
        shallowfeatvec = F.normalize(shallowfeatvec, dim=-1)
    output.append(shallowfeatvec * params["shallow_weight"])

    stg2fusevec, stg2imagevec, _, stg2voxvec = nets.stage2_fuse_block_add(
        imagefeatmap, output[-1], data_dict["stg2voxvec"], data_dict["voxvec_fuse"], params, "stg2fuseblock.", opt, False, None,
        voxmap=voxmap)
    stg2fusevec = F.linear(stg2fusevec, params["stg2fusefc.weight"], params["stg2fusefc.bias"])

    final = []
    ft = opt.final_type if isinstance(opt.final_type, (list, tuple)) else opt.final_type.split("_")
    for name, vec, wname in (("imageorg", imagefeatvec_org, "imageorg_weight"), ("voxorg", voxfeatvec_org, "voxorg_weight"),
                             ("shalloworg", shallowfeatvec, "shalloworg_weight"), ("stg2image", stg2imagevec, "stg2image_weight"),
                             ("stg2vox", stg2voxvec, "stg2vox_weight"), ("stg2fuse", stg2fusevec, "stg2fuse_weight")):
        if name in ft:
            final.append(vec * params[wname])
    if opt.final_fusetype == "add":
        x = sum(final)
    elif opt.final_fusetype == "cat":
        x = torch.cat(final, dim=-1)
    elif opt.final_fusetype == "catadd":
        x = torch.cat(final[:-1], dim=-1) + final[-1]
    else:
        raise NotImplementedError(opt.final_fusetype)
    if opt.final_l2:
        x = F.normalize(x, dim=-1)
    return {"imagevec_org": imagefeatvec_org, "voxvec_org": voxfeatvec_org, "shallowvec_org": shallowfeatvecorg,
            "stg2fusevec": stg2fusevec, "stg2imagevec": stg2imagevec, "stg2voxvec": stg2voxvec, "embedding": x}


def cast(d, dtype):
    """A data dict's floating tensors in `dtype` (coords keep their values: small integers)."""
    out = {}
    for k, v in d.items():
        if isinstance(v, (list, tuple)):
            out[k] = [t.to(dtype) for t in v]
        elif torch.is_tensor(v) and v.is_floating_point():
            out[k] = v.to(dtype)
        else:
            out[k] = v
    return out
