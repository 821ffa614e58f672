"""Host -> device input staging.

The reference moves every tensor of a batch to the GPU synchronously at the top of the step
(`data_dict[k] = v.to(args.device)`, train.py:303-304) after its DataLoader workers have decoded, resized, normalised
(fp32) and width-concatenated the camera tiles on the CPU (datasets/datasets_ws_nuscenes.py:604-634).  Here the host
ships the decoded uint8 tiles (4x fewer bytes than the normalised fp32 panorama) and the device does the rest
(ops.pack_cameras_u8 -> agp_pack_u8_cams_to_nhwc); this module is the transport:

    PinnedRing   `depth` slots, each a pinned host buffer + a device buffer per named tensor.  `upload(slot)` enqueues
                 the slot's H2D copies on a dedicated COPY stream (after the consumer of the slot's previous contents
                 has released it); `acquire(slot)` makes the caller's stream wait for that upload and returns the device
                 tensors; `release(slot)` marks them consumed.  With depth >= 2 the upload of batch i+1 runs under the
                 compute of batch i: PCIe never sits in the step's critical path as long as a batch's bytes move faster
                 than the step computes (57.8 MB of uint8 tiles per 64 panoramas: 0.9 ms at PCIe 5 x16 against a 2.4 ms step).

Measured on the MI355X box (round 2, bench.py --h2d, 67.4 MB of uint8 tiles per 64-pair step): resident inputs 2.42 ms per
step, this ring 2.8 - 2.9 ms.  The copy itself is not the bound (hipMemcpyAsync of 64 MB: 1.24 ms = 54 GB/s, and ring depth
2, 3, 4 give the same step); running it beside the step costs: every kernel of the step gets ~4.5 % slower (rocprofv3
kernel trace with / without the copy) and the rest is launch latency (AQL packets and completion signals cross the same
PCIe link the bulk read saturates).  Tried and rejected: splitting the upload into 8 copies (3.3 ms), blit copies
(HSA_ENABLE_SDMA=0: 3.7 ms), a bounded-grid copy kernel reading the pinned arena (8 workgroups: 2.75 ms, more are worse),
packing straight from the pinned arena (zero-copy: 3.9 ms -- PCIe-stalled waves take the convolutions' wave slots).

Loader workers write straight into `ring.host(slot)[name]` (pinned, page-locked: `torch.from_numpy` views of it can be
handed to worker processes through shared memory); nothing here touches pixel values.

The lidar half of a query ships as raw scans (`points` [N,3] + `point_offsets` [B+1]; quantisation, deduplication and the
augmentation rotation run on the device: SparseTensor.from_points_capacity); `random_z_rotation` draws the
rotation the reference's collate function applies on the CPU.

The camera half can ship one step earlier still: the DECODED frames as they leave the image decoder (`query_frames`
[b,ncam,H0,W0,3], `db_frames`), resized on the device (ops.pack_cameras_resized_u8).  PinnedRing needs no change
for that: a slot's tensors have whatever shapes the caller names, so a ring of frames is a ring with larger uint8 entries.
"""
import math

import torch


def z_rotation(theta):
    """fp32 [3,3]: the reference's PCRandomRotation._M((0, 0, 1), theta) = expm(np.cross(np.eye(3), (0, 0, theta))) in closed
    form, [[cos t, -sin t, 0], [sin t, cos t, 0], [0, 0, 1]] (evaluated in double precision, rounded once); applied to ROW
    vectors, `coords @ R`."""
    c, s = math.cos(theta), math.sin(theta)
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64).to(torch.float32)


def random_z_rotation(max_theta_deg=5.0, generator=None):
    """The matrix of the reference's collate-time augmentation PCRandomRotation(max_theta=max_theta_deg, max_theta2=0, axis=z)
    (datasets_ws_nuscenes.py:141): an angle drawn uniformly from +-max_theta_deg about z (max_theta2 = 0 makes the second
    factor the identity).  Host arithmetic; pass the result as data_dict['pc_rotation'] (MM.forward_q) or `rotation=`."""
    u = float(torch.rand(1, generator=generator, dtype=torch.float64))
    return z_rotation((math.pi * max_theta_deg / 180.0) * 2.0 * (u - 0.5))


def _jitter_range(name, value, center, lo_bound, hi_bound, clip_at_zero):
    """torchvision's ColorJitter._check_input for a number: [center - v, center + v], the first three clamped at 0; None when the
    range is the single point `center` (the op is then left out and draws nothing)."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0.0 <= value < float("inf")):
        raise ValueError(f"color_jitter: {name} {value!r} must be a finite number >= 0")
    lo, hi = center - float(value), center + float(value)
    if clip_at_zero:
        lo = max(lo, 0.0)
    if not (lo_bound <= lo <= hi <= hi_bound):
        raise ValueError(f"color_jitter: {name} values must lie in [{lo_bound}, {hi_bound}], got [{lo}, {hi}]")
    return None if lo == hi == center else (lo, hi)


def color_jitter(n, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, generator=None):
    """n parameter records of torchvision's ColorJitter(brightness, contrast, saturation, hue) as float32 [n, 8] on the CPU --
    `.cuda()` it and pass it as data_dict['query_jitter'] / ['db_jitter'] beside the frames (one record per frame, in the
    frames' memory order), or to ops.jitter_cameras_u8.  The reference's loaders call ColorJitter(j, j, j, hue=min(0.5, j))
    (datasets_ws_kitti360.py:236-280; Options.q_jitter / db_jitter hold j).

    A record: [0:4] the ops in the order they run (0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue), [4:7] the brightness,
    contrast and saturation factors, [7] the hue byte shift.  Per frame the draws are ColorJitter.get_params', in its order and with
    its torch calls: torch.randperm(4), then torch.empty(1).uniform_(lo, hi) for brightness, contrast, saturation and hue; an op whose
    range is a single point draws nothing and is marked absent (0 in its slot of the order).  Ranges: a value v gives
    [max(0, 1 - v), 1 + v] for the first three and [-v, v], 0 <= v <= 0.5, for hue.

    The hue byte shift is int(hue_factor * 255) truncated toward zero, mod 256.  This is the PINNED definition of the wrap-around
    in torchvision's PIL path, `np_h += np.uint8(hue_factor * 255)` on the uint8 H channel: a negative factor -f shifts by
    256 - int(f * 255)."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"color_jitter: n {n!r} must be a non-negative integer")
    ranges = [_jitter_range("brightness", brightness, 1.0, 0.0, float("inf"), True),
              _jitter_range("contrast", contrast, 1.0, 0.0, float("inf"), True),
              _jitter_range("saturation", saturation, 1.0, 0.0, float("inf"), True),
              _jitter_range("hue", hue, 0.0, -0.5, 0.5, False)]
    out = torch.zeros((n, 8), dtype=torch.float32)
    out[:, 4:7] = 1.0
    for i in range(n):
        order = torch.randperm(4, generator=generator)
        vals = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1], generator=generator)) for r in ranges]
        for k, fn in enumerate(order.tolist()):
            if vals[fn] is not None:
                out[i, k] = fn + 1
        for fn in range(3):
            if vals[fn] is not None:
                out[i, 4 + fn] = vals[fn]
        if vals[3] is not None:
            out[i, 7] = int(vals[3] * 255) % 256
    return out


class PinnedRing:
    def __init__(self, spec, depth=2, device="cuda"):
        """spec: {name: (shape, dtype)} of one batch."""
        if depth < 1:
            raise ValueError("PinnedRing: depth >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PinnedRing stages into GPU memory (agplace_amd has no CPU path)")
        self.depth = depth
        # ONE pinned arena and ONE device arena per slot, the named tensors are views into them: a slot uploads as a
        # single copy (measured on the MI355X box: a 64 MB pinned copy moves at 35 GB/s, an 8 MB one at 11 GB/s --
        # two copies per step, 58 MB + 10 MB, were slower than the step they should hide under)
        offs, total = {}, 0
        for k, (shape, dt) in spec.items():
            nbytes = int(torch.Size(shape).numel()) * torch.empty((), dtype=dt).element_size()
            offs[k] = (total, nbytes, tuple(shape), dt)
            total = (total + nbytes + 255) // 256 * 256
        self._harena = [torch.empty(total, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self._darena = [torch.empty(total, dtype=torch.uint8, device=self.device) for _ in range(depth)]

        def views(arena):
            return {k: arena[o:o + n].view(dt).view(shape) for k, (o, n, shape, dt) in offs.items()}
        self._host = [views(a) for a in self._harena]
        self._dev = [views(a) for a in self._darena]
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._ready = [torch.cuda.Event() for _ in range(depth)]      # upload of the slot has finished
        self._free = [torch.cuda.Event() for _ in range(depth)]       # the consumer has finished with the slot's device tensors
        self._free_valid = [False] * depth
        self.bytes_per_batch = total

    def host(self, slot):
        """The slot's pinned host tensors: the producer (dataloader) fills them in place."""
        return self._host[slot % self.depth]

    def device_tensors(self, slot):
        """The slot's device tensors (static addresses for the life of the ring: a captured hipGraph may bake them in).
        Use `acquire` to also order a stream behind the slot's upload."""
        return self._dev[slot % self.depth]

    def host_arena(self, slot):
        """The slot's whole pinned buffer / device buffer as flat uint8 tensors (one copy moves a slot)."""
        return self._harena[slot % self.depth]

    def device_arena(self, slot):
        return self._darena[slot % self.depth]

    def upload(self, slot):
        """Enqueue host -> device copies of the slot on the copy stream (asynchronous; returns at once)."""
        s = slot % self.depth
        with torch.cuda.stream(self.copy_stream):
            if self._free_valid[s]:
                self.copy_stream.wait_event(self._free[s])          # do not overwrite tensors a kernel may still read
            self._darena[s].copy_(self._harena[s], non_blocking=True)
            self._ready[s].record(self.copy_stream)

    def acquire(self, slot, stream=None):
        """Device tensors of the slot, valid on `stream` (default: the current stream) once its upload has landed."""
        s = slot % self.depth
        (stream or torch.cuda.current_stream(self.device)).wait_event(self._ready[s])
        return self._dev[s]

    def release(self, slot, stream=None):
        """The work enqueued so far on `stream` is the last reader of the slot's device tensors."""
        s = slot % self.depth
        self._free[s].record(stream or torch.cuda.current_stream(self.device))
        self._free_valid[s] = True
