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
"""
import contextlib

import torch

from . import _lib


def active(opt, prec, train):
    """Whether a forward at MFMA precision `prec` binds the guard: inference on fp16 maps (modes 2 / 4) with the option on."""
    return bool(getattr(opt, "fp16_range_guard", False)) and not train and prec in (2, 4)


def active_train(opt):
    """Whether a forward on the TRAINING graph binds the guard (Options.train_range_guard), in either train_precision mode: the
    fast mode's z16 / y16 planes and, in both modes, the fp16 operand planes of the one-pass weight gradient."""
    return bool(getattr(opt, "train_range_guard", False))


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
        try:
            yield w
        finally:
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
def guarded(model, opt, prec, train):
    """Around a model's inference work: bind its guard when active(opt, prec, train), publish behind the work on exit."""
    if not active(opt, prec, train):
        yield
        return
    g, dev = guard_of(model), model_device(model)
    with g.bind(dev):
        yield
    g.publish(dev, prec)


@contextlib.contextmanager
def guarded_train(model, opt):
    """Around a model's forward on the TRAINING graph (not its backward, which stores no fp16 map): bind the model's one guard
    when active_train(opt), publish behind the forward on exit -- the same word, mirrors and capture rules as guarded()."""
    if not active_train(opt):
        yield
        return
    g, dev = guard_of(model), model_device(model)
    with g.bind(dev):
        yield
    g.publish(dev, train_tag(opt))


def poll(model):
    g = model.__dict__.get('_fp16_guard')
    if g is not None:
        g.poll()


def ok(model):
    g = model.__dict__.get('_fp16_guard')
    return True if g is None else g.ok()
