"""fp64 CPU reference of MM.forward_q on the ConvNeXt-tiny trunk IN TRAINING (test infrastructure).

`forward_q` of tests/mm_convnext_ref.py restated with two differences: `training` / `pattern` reach nets.stage2_fuse_block_add and
the sparse oracle (batch-statistics BatchNorm, imposed ReLU masks), and the image maps are computed WITH autograd through
convnext_train_ref.forward_maps_scaled(trunk, image, scales) -- `scales` being the per-block stochastic-depth factors the product
drew (ConvNeXt.last_row_scales), or None.  tests/test_mm_convnext_train_host.py pins the restatement: with training=False and no
scales it returns mm_convnext_ref.forward_q's outputs exactly.
"""
import torch
import torch.nn.functional as F

import convnext_train_ref
from oracle import nets


def adopt_trunk(params, layers):
    """The restated trunk (tests/convnext_ref.py) holding the image_fe.fe.* values of `params`, in their dtype; the entries of
    `params` under image_fe.fe.features.* are REPLACED by the trunk's own Parameters (requiring gradients), so that one backward
    through forward_q leaves every gradient, the trunk's included, in `params[...] .grad`.  Returns the trunk."""
    import convnext_ref
    pre = "image_fe.fe."
    dtype = params[pre + "features.0.0.weight"].dtype
    trunk = convnext_ref.trunk([int(v) for v in layers]).to(dtype).eval()
    trunk.load_state_dict({k[len(pre):]: v.detach() for k, v in params.items() if k.startswith(pre)}, strict=True)
    for k, p in trunk.named_parameters():
        p.requires_grad_(k.startswith("features."))
        params[pre + k] = p
    return trunk


def forward_q(data_dict, params, opt, trunk, scales=None, training=False, pattern=None):
    """The seven outputs of MM.forward_q.  trunk: the fp64 restatement whose parameters are (or alias) params['image_fe.fe.*'];
    scales: one [n] tensor or None per block, stage by stage; training / pattern: as oracle.nets.mm_forward_q."""
    image = data_dict["query_image"]
    maps = convnext_train_ref.forward_maps_scaled(trunk, image, scales)
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
                                            training=training, pattern=pattern, num_top_down=getattr(opt, "mm_voxfe_ntd", 0))
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
        imagefeatmap, output[-1], data_dict["stg2voxvec"], data_dict["voxvec_fuse"], params, "stg2fuseblock.", opt, training, pattern,
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
