"""The fp16 range guard (Options.fp16_range_guard): report feature maps that left fp16's range.

Precision modes 2 and 4 store every feature map as fp16 and the conv epilogues clamp each value to +-65504 before the
conversion (csrc/common.hpp), so a map beyond fp16's range saturates silently.  While a device word is BOUND to the calling
host thread (agp_range_flag_set, include/agplace_hip.h), every guarded kernel that had to clamp a value ORs 1 into that word.
The stored values are the same bits with and without a binding.  With map exponents installed
(agplace_amd/map_exponents.py) a map is stored times 2^-e and the guard keeps watching the stored values: it then reports only
what the calibration did not cover.

One Guard per model: one sticky int32 word per device, one pinned host mirror and one event per launching stream.  After a
guarded forward, publish() enqueues a non-blocking copy of the word to the stream's mirror; captured into a hipGraph that copy
is a node of the graph, so every REPLAY publishes its own state and poll() reads the mirrors without touching a stream.

The word and the mirrors are made OUTSIDE any capture (at the first guarded eager forward on a device / stream): pinned memory
is never allocated inside a capture, and a first guarded forward inside one raises RuntimeError.  A capture stream that has no
mirror of its own takes the spare mirror the last eager forward on the device left behind.  The word is zeroed with an
elementwise kernel (mul_(0)) after a device synchronisation, never with a memset next to replayed graphs (mm.py, _vox_slot).

Training (Options.train_range_guard, guarded_train): forwards on the training graph store fp16 too -- the fast mode's z16 / y16
planes and, in both train_precision modes, the fp16 operand planes of the one-pass weight gradient (DESIGN.md section 2 lists
every store).  The same Guard of the model is bound around the training FORWARD only (the backward stores no fp16 map) and
published behind it; the report then says that a training forward saturated.  The guard reports, it does not rescue.

The ConvNeXt trunk's precision 4 (Options.convnext_range_guard, guarded_cnx / cnx_tag): its inference kernels round six MFMA
operands to fp16 -- a block's LayerNorm output, the GELU output and a downsample's LayerNorm output in the kernels (guarded twins of
csrc/convnext.hip, which read the bound word like every other guarded kernel), W1, W2 and the downsample weight on the host when
the planes are prepared (convnext._half).  A prepared plane cannot report through a kernel, so it carries a device-side int32 flag
(computed with tensor ops when the plane is made, no read-back); a forward that uses the planes under a binding hands the flag to
the bound guard (note_planes, through the thread-local that bind() sets) and publish() ORs it into the word with an elementwise
kernel on the calling stream -- there, because the calling stream has joined its side streams by then, so no kernel's atomic OR
can fall between that kernel's read and its write; captured, the OR is a node of the graph and every replay reports the planes
again.  The report carries the tag "cnx4"; "cnx4+2" / "cnx4+4" when the same word also covers fp16 maps of mfma_precision 2 / 4
(MM with both switches).
"""
import contextlib
import threading

import torch

from . import _lib


def active(opt, prec, train):
    """Whether a forward at MFMA precision `prec` binds the guard: inference on fp16 maps (modes 2 / 4) with the option on."""
    return bool(getattr(opt, "fp16_range_guard", False)) and not train and prec in (2, 4)


def active_train(opt):
    """Whether a forward on the TRAINING graph binds the guard (Options.train_range_guard), in either train_precision mode: the
    fast mode's z16 / y16 planes and, in both modes, the fp16 operand planes of the one-pass weight gradient."""
    return bool(getattr(opt, "train_range_guard", False))


def active_cnx(opt, fe_precision, train=False):
    """Whether an INFERENCE forward of a ConvNeXt trunk at precision `fe_precision` binds the guard (Options.convnext_range_guard):
    precision 4 only; precision 3 and every training forward (mode 3 whatever is set) store no fp16 and bind nothing."""
    return bool(getattr(opt, "convnext_range_guard", False)) and not train and fe_precision == 4


def cnx_tag(opt, fe_precision, maps_prec=None):
    """What a guarded ConvNeXt inference forward publishes as its `prec` (Guard.last_prec), or None when active_cnx() is false:
    "cnx4" = the trunk's precision-4 operands alone; "cnx4+2" / "cnx4+4" = one word over the trunk AND the fp16 maps a model stores
    at mfma_precision `maps_prec` with fp16_range_guard on (MM: stage 2 and the voxel branch)."""
    if not active_cnx(opt, fe_precision):
        return None
    return f"cnx4+{maps_prec}" if maps_prec is not None and active(opt, maps_prec, False) else "cnx4"


_tls = threading.local()           # .bound: (Guard, word tensor) of the innermost Guard.bind of this host thread, or None


def bound_word():
    """The int32 [1] device word Guard.bind bound for the calling host thread (the tensor behind agp_range_flag_get), or None."""
    b = getattr(_tls, "bound", None)
    return None if b is None else b[1]


def note_planes(flag):
    """A forward uses host-prepared fp16 planes whose clamp flag is `flag` (int32 [1] on the device, non-zero: an element was
    clamped): under a binding the bound guard ORs it into its word at its next publish(); without one nothing happens."""
    b = getattr(_tls, "bound", None)
    if b is not None and flag is not None and flag.device == b[1].device:
        b[0]._pending[id(flag)] = flag


# what a training forward publishes as its `prec` (Guard.last_prec): "train16" = the fast mode, "train32" = the tight mode
def train_tag(opt):
    return f"train{getattr(opt, 'train_precision', 32)}"


class Guard:
    def __init__(self, owner):
        self.owner = owner          # the model's name in messages
        self._words = {}            # str(device) -> int32 [1] device tensor
        self._spare = {}            # str(device) -> pinned int32 [1], the mirror a capture stream takes
        self._slots = {}            # (str(device), stream handle) -> {'host', 'event', 'calls'}
        self.last_prec = None
        self.also = set()           # other sources whose maps this word covers (pair.embed_pair: the other model's trunks)
        self._pending = {}          # id -> clamp flag of host-prepared fp16 planes used since the last publish (note_planes)

    # ---- storage (eager only)
    def _word(self, dev):
        key = str(dev)
        w = self._words.get(key)
        if w is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self.owner}: the fp16 range guard's device word is made by the first guarded EAGER forward on "
                                   f"{key}; run one forward of this model outside the capture first")
            w = torch.zeros(1, dtype=torch.int32, device=dev)
            self._words[key] = w
        if key not in self._spare and not torch.cuda.is_current_stream_capturing():
            self._spare[key] = torch.zeros(1, dtype=torch.int32).pin_memory()
        return w

    def _slot(self, dev):
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
        sl = self._slots.get(key)
        if sl is None:
            if torch.cuda.is_current_stream_capturing():
                host = self._spare.pop(str(dev), None)
                if host is None:
                    raise RuntimeError(f"{self.owner}: no pinned mirror is left for this capture stream; run one guarded forward of "
                                       "this model outside the capture first")
            else:
                host = torch.zeros(1, dtype=torch.int32).pin_memory()
            sl = self._slots[key] = {'host': host, 'event': None, 'calls': 0}
        return sl

    @contextlib.contextmanager
    def bind(self, dev):
        """Bind this guard's word on `dev` for the calling host thread; the previous binding is restored on exit."""
        w = self._word(dev)
        lib = _lib.load()
        prev = lib.agp_range_flag_set(w.data_ptr())
        prev_bound = getattr(_tls, "bound", None)
        _tls.bound = (self, w)      # the same binding for Python callers (bound_word, note_planes)
        try:
            yield w
        finally:
            _tls.bound = prev_bound
            lib.agp_range_flag_set(prev)

    def publish(self, dev, prec):
        """Behind the guarded work, on the calling stream (which has joined its side streams): the sticky word -> the stream's
        pinned mirror.  Eager calls also check, as MM._publish_voxel_flag does: the first call of a stream its own state at once,
        every later call the state the call BEFORE it published -- a bad batch is reported one call late, the last one of a loop
        by ok()."""
        self.last_prec = prec
        w = self._word(dev)
        sl = self._slot(dev)
        capturing = torch.cuda.is_current_stream_capturing()
        pending, self._pending = self._pending, {}
        for flag in pending.values():
            if flag.device == w.device:
                w.bitwise_or_(flag)        # an elementwise kernel on the calling stream, never a memset (module docstring)
        if not capturing and sl['event'] is not None:
            sl['event'].synchronize()
            if int(sl['host'][0]) != 0:
                self.report("the previous")
        sl['host'].copy_(w, non_blocking=True)
        if capturing:
            return
        sl['event'] = torch.cuda.Event()
        sl['event'].record(torch.cuda.current_stream(dev))
        sl['calls'] += 1
        if sl['calls'] == 1:
            sl['event'].synchronize()
            if int(sl['host'][0]) != 0:
                self.report("this")

    def poll(self):
        """NON-BLOCKING: raise ValueError if a published state seen so far (eager or replayed) holds a saturated map."""
        for sl in self._slots.values():
            if int(sl['host'][0]) != 0:
                self.report("an earlier")

    def ok(self):
        """False if any guarded forward since the last report or reset stored a saturated value.  Synchronises the device."""
        if not self._words:
            return True
        torch.cuda.synchronize()
        return all(int(w.item()) == 0 for w in self._words.values())

    def reset(self):
        torch.cuda.synchronize()
        for w in self._words.values():
            w.mul_(0)          # an elementwise kernel, not a memset (see the module docstring)
        for sl in self._slots.values():
            sl['host'].zero_()
            sl['event'] = None
        torch.cuda.synchronize()

    def report(self, which):
        self.reset()           # the error is reported once: start again from zero
        prec = self.last_prec
        also = "".join(f"; this report also covers {a}" for a in sorted(self.also))
        if isinstance(prec, str) and prec.startswith("cnx4"):
            maps = prec[5:]         # "" | the mfma_precision whose fp16 maps the same word covers
            both = (f" -- or, since this word also covers them, a feature map of precision mode {maps} (stage 2, the voxel branch) "
                    "left fp16's range (|v| > 65504) and was stored saturated" if maps else "")
            fix = (f"; if the saturated value was a feature map, Options.mfma_precision = 3 (split-bf16 maps, fp32 range) is the "
                   "remedy for it" if maps else "")
            raise ValueError(f"{self.owner}: in {which} batch an operand of the ConvNeXt trunk's precision-4 products "
                             "(Options.convnext_precision = 4) was stored saturated (|v| > 65504 before the clamp): a block's "
                             "LayerNorm output, the GELU output, a downsample's LayerNorm output, or an fp16 weight plane (W1, W2, "
                             f"the downsample weight){both}. The trunk's maps and everything computed from them are wrong{also}. The "
                             "guard reports, it does not rescue: run this trunk with Options.convnext_precision = 3 (bf16 pairs, "
                             f"fp32 range){fix}")
        if isinstance(prec, str) and prec.startswith("train"):
            raise ValueError(f"{self.owner}: in {which} batch a training forward (Options.train_precision = {prec[5:]}) stored an fp16 "
                             "value saturated (|v| > 65504 before the clamp): a pre-BatchNorm plane or a conv1 -> conv2 plane of the "
                             "fast mode, or an fp16 operand plane of the one-pass weight gradient (DESIGN.md section 2). The step "
                             f"trained on clamped activations or clamped weight-gradient operands{also}. The guard reports, it does "
                             "not rescue: lower the weights' / BatchNorm gammas' scale, or train this model in the tight mode "
                             "(train_precision = 32), whose maps are split-bf16")
        raise ValueError(f"{self.owner}: in {which} batch a feature map left fp16's range (|v| > 65504) and was stored saturated in "
                         f"precision mode {prec}: its outputs are wrong{also}. Run this model with Options.mfma_precision = 3 "
                         "(split-bf16 maps, fp32 range). For the image path agplace_amd.map_exponents.calibrate chooses per-map "
                         "power-of-two exponents that keep such a checkpoint in this mode; the guard watches the STORED values, so "
                         "with exponents installed it reports what the calibration did not cover")


def guard_of(model):
    g = model.__dict__.get('_fp16_guard')
    if g is None:
        g = model.__dict__['_fp16_guard'] = Guard(type(model).__name__)
    return g


def model_device(model):
    for p in model.parameters():
        return p.device
    return torch.device("cuda", torch.cuda.current_device())


@contextlib.contextmanager
def _guarded(model, tag, publish=True):
    """The one body of the context managers below.  `tag` None: nothing is bound.  Otherwise bind the model's one guard around the
    work and, when `publish`, publish behind it under `tag` (not if the work raised)."""
    if tag is None:
        yield
        return
    g, dev = guard_of(model), model_device(model)
    with g.bind(dev):
        yield
    if publish:
        g.publish(dev, tag)


def guarded(model, opt, prec, train):
    """Around a model's inference work: bind its guard when active(opt, prec, train), publish behind the work on exit."""
    return _guarded(model, prec if active(opt, prec, train) else None)


def guarded_cnx(model, tag):
    """Around inference work that runs a ConvNeXt trunk at precision 4 (`tag` from cnx_tag; None: nothing is bound): bind the model's
    one guard, publish behind the work under `tag` -- the same word, mirrors and capture rules as guarded()."""
    return _guarded(model, tag)


def bound(model, on):
    """Bind the model's guard around a PART of its forward when `on`, publishing nothing: the caller publishes behind the whole
    forward (publish_tag), once its side streams have joined."""
    return _guarded(model, True if on else None, publish=False)


def publish_tag(model, tag):
    guard_of(model).publish(model_device(model), tag)


def guarded_train(model, opt):
    """Around a model's forward on the TRAINING graph (not its backward, which stores no fp16 map): bind the model's one guard
    when active_train(opt), publish behind the forward on exit -- the same word, mirrors and capture rules as guarded()."""
    return _guarded(model, train_tag(opt) if active_train(opt) else None)


def poll(model):
    g = model.__dict__.get('_fp16_guard')
    if g is not None:
        g.poll()


def ok(model):
    g = model.__dict__.get('_fp16_guard')
    return True if g is None else g.ok()
