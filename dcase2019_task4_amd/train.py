"""Mean-teacher train step on MI355X - host-side mirror of baseline/main.py:45-165.

Two ways in:

* drop-in: keep baseline/main.py's own ``train`` loop and ``torch.optim.Adam`` and just build the
  models with ``dcase2019_task4_amd.crnn.CRNN`` - forward/backward then run in the HIP kernels
  through one autograd node.  ``update_ema_variables`` below is the same call as main.py:45-49
  fused into one kernel over the flat parameter buffers.
* fused: ``MeanTeacherStep`` runs the whole body of the loop (main.py:84-157: teacher forward,
  student forward, losses, backward, Adam, EMA, step counter) as a fixed sequence of C-ABI calls
  on persistent buffers, optionally captured into one hipGraph, with every per-step scalar
  (consistency weight, EMA alpha, Adam bias correction, dropout seeds) advanced ON DEVICE - none
  of the ~11 host syncs per step of the reference loop (main.py:106-149 ``.item()``).  ``train``
  wraps it in the reference's epoch-loop signature.
"""
import ctypes as C
import os
import time

import numpy as np
import torch

from . import _lib
from . import dist as sdist
from .crnn import CRNN

LOSS_NAMES = ("loss", "weak_class_loss", "strong_loss", "cons_strong", "cons_weak", "weak_ema_loss",
              "strong_ema_loss", "cons_weight")


def update_ema_variables(model, ema_model, alpha, global_step):
    """main.py:45-49 - ``alpha = min(1 - 1/(global_step+1), alpha)``; parameters only (buffers are
    not averaged).  One fused kernel over the two flat buffers."""
    alpha = min(1 - 1 / (global_step + 1), alpha)
    model.flatten_parameters_()
    ema_model.flatten_parameters_()
    n = model._flat.numel()
    _lib.check(_lib.lib().sed_ema_update(n, _lib.ptr(model._flat), _lib.ptr(ema_model._flat), float(alpha),
                                         _lib.stream_ptr()), "sed_ema_update")


_STREAM_POOL = {}


def shared_stream(device, role, priority=0):
    """One torch stream per (device, role, priority) for the whole process.  Every stream a step hands to the library also gets
    two helper streams inside it (sed_stream_prepare); until round 5 nothing ever destroyed those, and a process that built
    several steps one after the other (bench.py's legs, a test session) ended up with dozens of live streams on four hardware
    queues - the graph branches of the later steps shared queues with them (measured: 0.90 instead of 0.66 ms for the fifth
    step built in a process).  The library now has sed_stream_release, and a step built with ``pool_streams=False`` owns its
    streams and releases them in ``close()``; the pool stays the default because steps of one process run one at a time and
    torch itself hands out streams from a fixed pool of 32 per device and priority."""
    key = (torch.device(device).index or 0, role, int(priority))
    st = _STREAM_POOL.get(key)
    if st is None:
        st = _STREAM_POOL[key] = torch.cuda.Stream(device=device, priority=int(priority))
    return st


def _slice_range(s, B):
    if s is None:
        return 0, 0
    lo, hi, st = s.indices(B)
    if st != 1:
        raise NotImplementedError("masks must be contiguous slices (main.py:241,247)")
    return lo, max(lo, hi)


class MeanTeacherStep:
    """The body of main.train's loop (main.py:84-157) as one fused, graph-capturable device step.

    ``teacher=None`` gives the supervised loop body of main_simple_CRNN.train (main_simple_CRNN.py:39-75):
    student forward, weak + strong BCE (either mask may be None), backward, Adam - no teacher forward, no
    consistency terms, no EMA."""

    def __init__(self, student, teacher, batch_size, n_frames, rampup_length, weak_mask, strong_mask, lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, ema_decay=0.999, max_consistency_cost=2.0, seed=0, use_graph=True,
                 process_group=None, overlap_streams=True, dp_schedule=None, pool_streams=True, collective=None):
        assert isinstance(student, CRNN) and (teacher is None or isinstance(teacher, CRNN))
        if not student.hot_path or (teacher is not None and not teacher.hot_path):
            raise _lib.SedError("MeanTeacherStep runs the HIP hot path only: this CRNN configuration is served by stock torch "
                                "operators (CRNN.hot_path is False) - use the reference's own loop for it")
        self.l = _lib.lib()
        self.student, self.teacher = student, teacher
        self.supervised = teacher is None
        dev = next(student.parameters()).device
        if dev.type != "cuda":
            raise _lib.SedError("MeanTeacherStep needs the models on the GPU (no CPU fallback)")
        self.device = dev
        student.flatten_parameters_(dev)
        if teacher is not None:
            teacher.flatten_parameters_(dev)
        self.B, self.T = int(batch_size), int(n_frames)
        if teacher is not None and (teacher._C, teacher._H, teacher._dtype) != (student._C, student._H, student._dtype):
            raise ValueError("student and teacher must have the same geometry and mfma_dtype")
        self.dims = student.make_dims(self.B, self.T)
        self._pool_streams = bool(pool_streams)
        self._owned_streams = []
        self.T3, self.NC = self.T // 8, student._nclass
        # the student's output heads are left to sed_mt_step_backward where the library runs them inside the backward recurrence
        # (csrc/kernels.h heads_fusable)
        self._defer_heads = (student._H == 64 and self.T3 <= 128)
        self.wlo, self.whi = _slice_range(weak_mask, self.B) if weak_mask is not None else (0, 0)
        self.slo, self.shi = _slice_range(strong_mask, self.B) if strong_mask is not None else (0, 0)
        n = student._flat.numel()
        self.n = n
        f32 = dict(device=dev, dtype=torch.float32)
        self.grads = torch.zeros(n, **f32)
        self.exp_avg = torch.zeros(n, **f32)
        self.exp_avg_sq = torch.zeros(n, **f32)
        self.state = torch.zeros(C.sizeof(_lib.SedStepState), device=dev, dtype=torch.uint8)
        self.steps_done = 0
        self._gs_offset = 0                # global_step_host = steps_done + _gs_offset: host mirror of state.global_step
        self.pg = process_group
        self.world, self.rank = 1, 0
        if process_group is not None:
            import torch.distributed as dist
            self.world = dist.get_world_size(process_group)
            self.rank = dist.get_rank(process_group)
        # every replica draws its OWN dropout masks / teacher noise: the rank is folded into the Philox base seed here
        # (rank 0 keeps the user's seed, so a one-process run and rank 0 of a data-parallel run see the same stream)
        self.seed_user = int(seed) & (2 ** 64 - 1)
        _lib.check(self.l.sed_step_state_init(_lib.ptr(self.state), self._folded_seed(), int(rampup_length),
                                              float(lr), float(betas[0]), float(betas[1]), float(eps),
                                              float(ema_decay), float(max_consistency_cost), _lib.stream_ptr()),
                   "sed_step_state_init")
        self.lr = float(lr)
        base = self.state.data_ptr()
        self._seed_s = C.c_void_p(base + _lib.SedStepState.seed_student.offset)
        self._seed_t = C.c_void_p(base + _lib.SedStepState.seed_teacher.offset)
        self.ctx_bytes = self.l.sed_crnn_ctx_bytes(C.byref(self.dims))
        self.ws_bytes = self.l.sed_crnn_bwd_ws_bytes(C.byref(self.dims))
        if self.ctx_bytes == 0 or self.ws_bytes == 0:
            raise _lib.SedError(self.l.sed_last_error().decode())
        # the library initialises what it needs initialised in fresh buffers (the wide model's cluster recurrence keeps
        # launch epochs, tagged exchange granules and its sticky timeout counter in there): sed_crnn_buffers_init
        self.ctx_s = _lib.scratch(self.ctx_bytes, dev)
        self.ctx_t = _lib.scratch(self.ctx_bytes if teacher is not None else 0, dev)
        self.ws = _lib.scratch(self.ws_bytes, dev)
        _lib.check(self.l.sed_crnn_buffers_init(C.byref(self.dims), _lib.ptr(self.ctx_s), self.ctx_bytes, _lib.ptr(self.ws),
                                                self.ws_bytes, _lib.stream_ptr()), "sed_crnn_buffers_init")
        if teacher is not None:
            _lib.check(self.l.sed_crnn_buffers_init(C.byref(self.dims), _lib.ptr(self.ctx_t), self.ctx_bytes, None, 0,
                                                    _lib.stream_ptr()), "sed_crnn_buffers_init")
        self._err_view = None
        if student._H == 256:
            off, nb = C.c_size_t(), C.c_size_t()
            _lib.check(self.l.sed_crnn_ctx_view(C.byref(self.dims), b"gru_err", C.byref(off), C.byref(nb)), "sed_crnn_ctx_view")
            self._err_view = (off.value, nb.value)
        self.x = torch.zeros(self.B, 1, self.T, 64, **f32)
        self.x_ema = torch.zeros(self.B, 1, self.T, 64, **f32)
        self.target = torch.zeros(self.B, self.T3, self.NC, **f32)
        self.strong = torch.empty(self.B, self.T3, self.NC, **f32)
        self.weak = torch.empty(self.B, self.NC, **f32)
        # supervised: the "teacher" outputs ARE the student's, so both consistency terms and their gradients are
        # exactly zero and the loss kernel needs no second variant
        self.strong_ema = torch.empty(self.B, self.T3, self.NC, **f32) if teacher is not None else self.strong
        self.weak_ema = torch.empty(self.B, self.NC, **f32) if teacher is not None else self.weak
        self.d_strong = torch.empty(self.B, self.T3, self.NC, **f32)
        self.d_weak = torch.empty(self.B, self.NC, **f32)
        self.losses = torch.zeros(8 + 8 * self.B + 8, **f32)          # SED_LOSS_FLOATS(B): meters | scratch
        # Data-parallel schedule (SED_FORCE_DP=1 takes it with a one-rank group too, so that the whole RCCL path can be
        # exercised on a single-GPU box).
        #   "overlap" (default): forward + loss + backward of heads/GRU (parts 5) | on a second stream: the tail bucket's
        #       weight-gradient GEMMs (parts 8) then its all-reduce, OVERLAPPING | the conv-block backward (parts 2) on the
        #       main stream | all-reduce of the conv bucket | Adam + EMA.  The GRU weight-gradient GEMMs stay off the
        #       critical path (they used to be on it in round 1's "split" schedule: +70 us), and 60 % of the gradient
        #       bytes cross xGMI while the conv backward (the longest part of the backward) is still computing.
        #   "single": whole backward (parts 3) | ONE all-reduce of the flat gradient buffer | update.  Nothing overlaps.
        #   SED_DP_CAPTURE=1 (RCCL only): the collectives are captured INTO the hipGraph, the whole step is one replay.
        self.dp = process_group is not None and (self.world > 1 or os.environ.get("SED_FORCE_DP") == "1")
        # Default: the overlap schedule with the collectives CAPTURED into the step's hipGraph when the backend is RCCL and a
        # trial capture of an all-reduce replays correctly on every rank (one replay per step; measured with a one-rank
        # RCCL group: 0.836 ms against 0.816 ms without data parallelism, 0.839 ms for "single", and 0.969 ms for the overlap
        # schedule with EAGER collectives between four graph segments - that one is host-bound: 4 graph launches + 2 async
        # collectives + stream waits per step).  Otherwise (gloo, or capture not available): "single" with an eager collective.
        self._cap_stream = self._stream("capture")
        # The gradient all-reduce itself: "p2p" = ONE kernel over peer-mapped device memory (dist.PeerAllReduce, csrc/p2p.hip:
        # reduce-scatter + all-gather with direct loads / stores between the ranks of a node, sums in rank order), "pg" = the
        # process group's all_reduce (RCCL, gloo), "auto" (default) = p2p when every rank can map every other one AND a
        # self-check against the process group's result passes on every rank, else pg.  The p2p launch is an ordinary kernel:
        # it is always capturable, and two ranks may share one GPU (RCCL refuses that), which is how the captured schedule is
        # tested at world 2 on a one-GPU box.
        # "auto" no longer stops at "p2p works": it TIMES both on the step's two buckets (50 captured replays each, MAX over the
        # ranks) and keeps the faster - dist.choose_collective; both sets of times go into self.collective_record (bench.py
        # prints them as config.dp_collective_record).
        want_coll = collective or os.environ.get("SED_DP_COLLECTIVE") or "auto"
        if want_coll not in ("auto", "p2p", "pg"):
            raise ValueError(f"unknown collective {want_coll!r}")
        self._buckets = sdist.grad_buckets(student._layout)
        self._p2p = None
        self.collective_record = None
        if self.dp and want_coll != "pg":
            if sdist.PeerAllReduce.aligned(self.grads, self._buckets + ((0, n),)):
                self._p2p = sdist.PeerAllReduce.create(n, dev, process_group)
            else:      # (never with the reference's parameter shapes: every tensor is a multiple of 4 floats)
                sdist.PeerAllReduce.last_error = "a gradient bucket does not start on a 16-byte boundary"
            if self._p2p is None and want_coll == "p2p":
                raise _lib.SedError(f"collective='p2p' is not available here: {sdist.PeerAllReduce.last_error}")
            if want_coll == "auto":
                choice, self.collective_record = sdist.choose_collective(self._p2p, self.grads, self._buckets, process_group, dev)
                if choice == "pg" and self._p2p is not None:
                    self._p2p.close()
                    self._p2p = None
        self.collective = "p2p" if self._p2p is not None else ("pg" if self.dp else None)
        env_cap = os.environ.get("SED_DP_CAPTURE")
        want = dp_schedule or os.environ.get("SED_DP_SCHEDULE")
        if want == "split":
            want = "overlap"
        if want not in (None, "overlap", "single"):
            raise ValueError(f"unknown data-parallel schedule {want!r}")
        self.dp_capture = False
        if self.dp and use_graph and env_cap != "0" and (want != "single" or env_cap == "1"):
            self.dp_capture = (env_cap == "1") or self._p2p is not None or self._collective_capture_works()
        self.dp_schedule = want or ("overlap" if (self.dp_capture or not self.dp) else "single")
        self._dp_stream = self._stream("collective") if self.dp else None
        # train_cnn=False (CRNN.py:18-20, main.py:289-290 filters the optimiser's parameters on requires_grad): the conv
        # blocks' backward is skipped and their gradient stays zero, which makes Adam's update of those entries exactly
        # zero (zero moments, no weight decay) while the EMA still covers every parameter (main.py:45-49 zips ALL of them)
        frozen = [not p.requires_grad for p in student.parameters()]
        self.cnn_frozen = all(frozen[:18]) and not any(frozen[18:])
        if any(frozen) and not self.cnn_frozen:
            raise NotImplementedError("MeanTeacherStep supports all parameters trainable, or the whole CNN frozen "
                                      "(train_cnn=False); other requires_grad patterns are not implemented")
        if process_group is not None:
            self.sync_replicas()
        self.use_graph = bool(use_graph)
        self.overlap = bool(overlap_streams)
        self._side = self._stream("teacher") if (self.overlap and teacher is not None) else None
        self._capture_error = None
        self._graph_a = None
        self._graph_w = None
        self._graph_c = None
        self._graph_b = None
        # graphs are captured on a stream of our own whose library helper stream exists BEFORE the capture starts
        for st in (torch.cuda.current_stream(dev), self._cap_stream, self._side, self._dp_stream):
            if st is not None:
                _lib.check(self.l.sed_stream_prepare(C.c_void_p(st.cuda_stream)), "sed_stream_prepare")
        self._warm = 0
        # Patch moments one step ahead (sed_crnn_moments, csrc/blk0.hip): block 0's train-mode BatchNorm statistics come from the
        # 9 + 45 moments of the 3x3 input patch, a function of the BATCH only.  When the batch in self.x / self.x_ema is still the
        # one the previous run() trained on (a resident batch: bench.py; anything that calls run() without load_batch() in
        # between), the previous step has already computed them - on a third stream beside its heads / BiGRU backward, which
        # leave most of the chip idle - and this step's forwards start at k_blk0_prep: 16 us (B = 24) off the head of the
        # critical chain, every step still computing one pair of moments.  step() / load_batch() + run() never speculates:
        # self.x may ONLY change through load_batch() (or be followed by invalidate_batch()).
        # Readiness belongs to the BATCH in self.x / self.x_ema, not to the step: whoever writes the moments into ctx marks them
        # valid (the tail below; a one-batch-ahead front-end's features()), whatever replaces the batch or the state clears
        # the mark (load_batch, invalidate_batch, load_state_dict), and run() picks its form from the mark alone.
        self.moments_ahead = False         # (off: measured slower for the resident-batch step; the hand-over tests set it)
        self._mom_valid = False            # ctx_s / ctx_t hold the moments of what is in self.x / self.x_ema right now
        self._resident = False            # a run() has consumed the batch in self.x and no load_batch() came since
        self._mom_ready = self._mom_next = False      # the variant being run / captured
        self._mom_stream = self._stream("moments")
        self._graph_sets = {}              # (mom_ready, mom_next) -> (graph_a, graph_w, graph_c, graph_b)

    @property
    def global_step_host(self):
        return self.steps_done + self._gs_offset

    def _stream(self, role, priority=0):
        if self._pool_streams:
            return shared_stream(self.device, role, priority)
        st = torch.cuda.Stream(device=self.device, priority=int(priority))
        self._owned_streams.append(st)
        return st

    def close(self):
        """Drops the graphs and releases what the library created for the streams this step OWNS (``pool_streams=False``):
        sed_stream_release destroys the two helper streams + events per stream.  Pooled streams are shared with every other
        step of the process and stay prepared.  The step must not be used afterwards."""
        torch.cuda.synchronize(self.device)
        self._graph_a = self._graph_w = self._graph_c = self._graph_b = None
        self._graph_sets = {}
        if self._p2p is not None:
            self._p2p.close()
            self._p2p = None
        for st in self._owned_streams:
            _lib.check(self.l.sed_stream_release(C.c_void_p(st.cuda_stream)), "sed_stream_release")
        self._owned_streams = []

    # ---- pieces ------------------------------------------------------------------------------------
    def _forward(self, model, x, ctx, seed, strong, weak):
        """strong = weak = None: output heads deferred to sed_mt_step_backward (the student's forward).  The teacher's forward is
        train-mode but never differentiated (main.py:87-89): train = 3 tells the library so."""
        train = 3 if (model is self.teacher and model is not None) else 1
        if self._mom_ready:
            train |= 4               # this batch's patch moments are already in ctx (the previous step's _moments_ahead)
        _lib.check(self.l.sed_crnn_forward(C.byref(self.dims), _lib.ptr(model._flat), _lib.ptr(model._bn_flat),
                                           _lib.ptr(model._bn_tracked), _lib.ptr(x), train, 1, seed, _lib.ptr(ctx),
                                           self.ctx_bytes, _lib.ptr(strong), _lib.ptr(weak), _lib.stream_ptr()),
                   "sed_crnn_forward")

    def _fwd_bwd(self, after_forward=None, at_recurrence=None):
        self._fork_exc = None
        try:
            self._fwd_bwd_impl(after_forward, at_recurrence)
        finally:
            if at_recurrence is not None:      # one-shot hook: never leave it registered (e.g. a forward that failed before it)
                self.l.sed_crnn_fork_callback(_lib.stream_ptr(), None, None)
        if self._fork_exc is not None:
            # ctypes swallows (prints) an exception raised inside a C callback: a failing hook - the next batch's feature
            # extraction - would otherwise leave a captured graph without those kernels and the step training on stale slots
            exc, self._fork_exc = self._fork_exc, None
            raise exc

    def _student_forward(self, at_recurrence):
        """The student forward (main.py:91).  The one-shot `at_recurrence` hook is registered right in front of THIS call: the
        library hands it to the next sed_crnn_forward on the stream, which without a side stream would be the teacher's."""
        if at_recurrence is not None:
            def hook(_user):
                try:
                    at_recurrence()
                except BaseException as e:      # noqa: BLE001 - re-raised by _fwd_bwd once the C call has returned
                    self._fork_exc = e
            self._fork_cb = _lib.FORK_CALLBACK(hook)      # (kept alive until the forward has run)
            _lib.check(self.l.sed_crnn_fork_callback(_lib.stream_ptr(), self._fork_cb, None), "sed_crnn_fork_callback")
        # the student's output heads are deferred where the library fuses them (n_RNN_cell = 64, T / 8 <= 128):
        # sed_mt_step_backward runs them with the loss and their backward inside the top layer's backward recurrence
        # (csrc/hfuse.h).  Other geometries (the 256-cell BiGRU) have no fused form: deferred, the student's k_heads_fwd would
        # queue up behind the teacher's AND the join (21 us of the wide step's critical chain); run by the forward it overlaps
        # the teacher's on the other stream.  Same kernels, same results.
        if self._defer_heads:
            self._forward(self.student, self.x, self.ctx_s, self._seed_s, None, None)
        else:
            self._forward(self.student, self.x, self.ctx_s, self._seed_s, self.strong, self.weak)

    def _fwd_bwd_impl(self, after_forward=None, at_recurrence=None):
        """teacher forward (main.py:87-89), student forward (:91), losses (:93-145), backward (:152-153).
        `after_forward`: called between the forwards and the backward; `at_recurrence`: called from INSIDE the student
        forward, between its conv stack and its recurrence (sed_crnn_fork_callback) - where the waveform front-end forks
        the next batch's feature kernels (features.WaveformFrontEnd)."""
        if self.supervised:
            self._student_forward(at_recurrence)
        elif self._side is not None:
            # the teacher forward is independent of the student forward: run it on a second stream
            cur = torch.cuda.current_stream()
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                self._forward(self.teacher, self.x_ema, self.ctx_t, self._seed_t, self.strong_ema, self.weak_ema)
            self._student_forward(at_recurrence)
            cur.wait_stream(self._side)
        else:
            self._forward(self.teacher, self.x_ema, self.ctx_t, self._seed_t, self.strong_ema, self.weak_ema)
            self._student_forward(at_recurrence)
        if after_forward is not None:
            after_forward()
        if self._mom_next:
            self._moments_ahead()
        # losses (main.py:93-145) + backward in one call: the heads-backward kernel forms the loss gradient per clip itself
        # (sed_mt_loss as a kernel of its own was 12 us on the critical path).  One process: the whole backward
        # (parts = 3), which lets the library overlap the GRU weight gradients with the conv-block backward;
        # data-parallel "split": part 1 here, part 2 after its bucket's all-reduce has been started (run())
        if self.cnn_frozen:
            parts = 1
        elif self.dp and self.dp_schedule == "overlap":
            parts = 5
        else:
            parts = 3
        if self._defer_heads:
            _lib.check(self.l.sed_mt_step_backward(C.byref(self.dims), _lib.ptr(self.student._flat), _lib.ptr(self.x),
                                                   self._seed_s, _lib.ptr(self.ctx_s), self.ctx_bytes,
                                                   _lib.ptr(self.strong), _lib.ptr(self.weak),
                                                   _lib.ptr(self.strong_ema), _lib.ptr(self.weak_ema), _lib.ptr(self.target),
                                                   self.wlo, self.whi, self.slo, self.shi, _lib.ptr(self.state), 1,
                                                   _lib.ptr(self.losses), None, None, _lib.ptr(self.grads),
                                                   _lib.ptr(self.ws), self.ws_bytes, parts, _lib.stream_ptr()),
                       "sed_mt_step_backward")
        else:
            _lib.check(self.l.sed_mt_loss_backward(C.byref(self.dims), _lib.ptr(self.student._flat), _lib.ptr(self.x),
                                                   self._seed_s, _lib.ptr(self.ctx_s), self.ctx_bytes,
                                                   _lib.ptr(self.strong_ema), _lib.ptr(self.weak_ema), _lib.ptr(self.target),
                                                   self.wlo, self.whi, self.slo, self.shi, _lib.ptr(self.state), 1,
                                                   _lib.ptr(self.losses), None, None, _lib.ptr(self.grads),
                                                   _lib.ptr(self.ws), self.ws_bytes, parts, _lib.stream_ptr()),
                       "sed_mt_loss_backward")

        if self._mom_next:
            torch.cuda.current_stream().wait_stream(self._mom_stream)

    def _moments_ahead(self, x=None, x_ema=None):
        """The patch moments of the batch the NEXT step trains on (default: the resident one in self.x / self.x_ema) into the
        models' ctx, on a stream of their own beside this step's backward."""
        cur = torch.cuda.current_stream()
        self._mom_stream.wait_stream(cur)
        with torch.cuda.stream(self._mom_stream):
            self._moments(self.x if x is None else x, self.ctx_s)
            if self.teacher is not None:
                self._moments(self.x_ema if x_ema is None else x_ema, self.ctx_t)

    def _moments(self, x, ctx):
        _lib.check(self.l.sed_crnn_moments(C.byref(self.dims), _lib.ptr(x), _lib.ptr(ctx), self.ctx_bytes, _lib.stream_ptr()),
                   "sed_crnn_moments")

    def invalidate_batch(self):
        """Tell the step that self.x / self.x_ema / self.target were written behind its back (anything but load_batch())."""
        self._mom_valid = False
        self._resident = False

    def _backward(self, parts):
        _lib.check(self.l.sed_crnn_backward(C.byref(self.dims), _lib.ptr(self.student._flat), _lib.ptr(self.x),
                                            self._seed_s, _lib.ptr(self.ctx_s), self.ctx_bytes,
                                            _lib.ptr(self.d_strong), _lib.ptr(self.d_weak), _lib.ptr(self.grads),
                                            _lib.ptr(self.ws), self.ws_bytes, parts, _lib.stream_ptr()), "sed_crnn_backward")

    def _update(self):
        """Adam (main.py:154) + EMA teacher (:155-157), one kernel."""
        _lib.check(self.l.sed_adam_ema(self.n, _lib.ptr(self.student._flat), _lib.ptr(self.grads),
                                       _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                                       _lib.ptr(self.teacher._flat) if self.teacher is not None else None,
                                       _lib.ptr(self.state), 1.0 / self.world,
                                       _lib.stream_ptr()), "sed_adam_ema")
        # (no sed_step_state_advance: the loss / heads-backward kernel of this step already moved the counters on and
        # left the update's own fields derived for this step - sed_mt_loss_backward(advance_state = 1))

    def _collective_capture_works(self):
        """Trial: capture one all-reduce into a hipGraph, replay it, compare with the eager result; every rank must succeed."""
        import torch.distributed as dist
        try:
            if dist.get_backend(self.pg) != "nccl":
                return False
            if self.world == 1:
                return True          # a one-rank all-reduce is a no-op: nothing to try
            t = torch.arange(1024, device=self.device, dtype=torch.float32) + self.rank
            ref = t.clone()
            dist.all_reduce(ref, group=self.pg)
            torch.cuda.synchronize(self.device)
            ok = 1.0
            try:
                g = torch.cuda.CUDAGraph()
                # thread_local: the process group's watchdog thread queries events of earlier collectives, which a
                # capture in the default "global" mode treats as an illegal call and aborts on
                with torch.cuda.graph(g, stream=self._cap_stream, capture_error_mode="thread_local"):
                    dist.all_reduce(t, group=self.pg)
                g.replay()
                torch.cuda.synchronize(self.device)
                ok = 1.0 if torch.equal(t, ref) else 0.0
            except Exception:
                ok = 0.0
            flag = torch.tensor([ok], device=self.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.pg)
            return bool(flag.item() == 1.0)
        except Exception:
            return False

    def _folded_seed(self):
        return sdist.fold_rank_seed(self.seed_user, self.rank)

    def sync_replicas(self, src=0):
        """Every replica starts from rank ``src``'s parameters, BatchNorm buffers, Adam moments and step counters (the
        reference has one copy of each; DDP convention: rank 0 wins) - e.g. after rank 0 loaded a checkpoint - and
        then re-folds its own rank into the dropout seed."""
        ts = [self.student._flat, self.student._bn_flat, self.student._bn_tracked, self.exp_avg, self.exp_avg_sq, self.state]
        if self.teacher is not None:
            ts += [self.teacher._flat, self.teacher._bn_flat, self.teacher._bn_tracked]
        sdist.broadcast_parameters(ts, self.pg, src=src)
        _lib.check(self.l.sed_step_state_update(_lib.ptr(self.state), self._folded_seed(), 0.0, 1, _lib.stream_ptr()),
                   "sed_step_state_update")
        self._gs_offset = int(self.read_state().global_step) - self.steps_done

    def set_global_step(self, global_step):
        """main.py:74 - ``global_step = epoch * len(train_loader) + i``: the reference recomputes the counter from the epoch
        argument on every call of ``train``; this sets the device counter the ramp-up, the EMA alpha and the dropout keys
        derive from (Adam's own step count is the optimiser's and stays)."""
        _lib.check(self.l.sed_step_state_set_global_step(_lib.ptr(self.state), int(global_step), _lib.stream_ptr()),
                   "sed_step_state_set_global_step")
        self._gs_offset = int(global_step) - self.steps_done

    def set_lr(self, lr):
        """Honour an optimiser whose lr changed between epochs (main.py never does; utils.adjust_learning_rate exists)."""
        if float(lr) != self.lr:
            self.lr = float(lr)
            _lib.check(self.l.sed_step_state_update(_lib.ptr(self.state), 0, self.lr, 2, _lib.stream_ptr()),
                       "sed_step_state_update")

    def _allreduce(self, lo, hi, async_op):
        if self._p2p is not None:                      # one kernel on the current stream; nothing to wait for on the host
            self._p2p.all_reduce(self.grads, lo, hi)
            return None
        return sdist.allreduce_bucket(self.grads, lo, hi, self.pg, async_op=async_op, force=True)

    def _dp_step_eager_collectives(self, graph):
        """One data-parallel step with the collectives issued between graph segments (any backend)."""
        (tlo, thi), (hlo, hhi) = self._buckets
        if self.dp_schedule == "single" or self.cnn_frozen:
            self._graph_a.replay() if graph else self._fwd_bwd()
            # synchronous form: this torch runs it on the CURRENT stream (no hop to the process group's own stream and back)
            if self.cnn_frozen:
                self._allreduce(tlo, thi, False)
            else:
                self._allreduce(0, self.n, False)
            self._graph_b.replay() if graph else self._update()
            return
        cur = torch.cuda.current_stream()
        self._graph_a.replay() if graph else self._fwd_bwd()                  # ... backward of heads + GRU (parts 5)
        self._dp_stream.wait_stream(cur)
        # second stream: weight gradients of the GRU + heads bucket, then that bucket's all-reduce - both while the main stream
        # runs the conv-block backward
        with torch.cuda.stream(self._dp_stream):
            self._graph_w.replay() if graph else self._backward(8)            # tail weight gradients (parts 8)
            w1 = self._allreduce(tlo, thi, True)                              # tail bucket over xGMI ...
        self._graph_c.replay() if graph else self._backward(2)                # ... while the conv blocks run backward
        # ONE collective in flight per communicator: the head bucket's all-reduce is issued only after the tail bucket's
        # has completed in stream order (it finished long before: the conv backward is ~350 us) - two collectives enqueued
        # from two streams on one communicator are otherwise ordered only by what the backend serialises internally
        with torch.cuda.stream(self._dp_stream):
            if w1 is not None:
                w1.wait()
        cur.wait_stream(self._dp_stream)
        w2 = self._allreduce(hlo, hhi, True)
        if w2 is not None:
            w2.wait()
        self._graph_b.replay() if graph else self._update()

    def _dp_step_body(self, after_forward=None, at_recurrence=None):
        """The same schedule as straight-line stream code (what SED_DP_CAPTURE=1 captures into ONE graph)."""
        (tlo, thi), (hlo, hhi) = self._buckets
        self._fwd_bwd(after_forward, at_recurrence)
        if self.dp_schedule == "single" or self.cnn_frozen:
            self._allreduce(tlo if self.cnn_frozen else 0, thi if self.cnn_frozen else self.n, False)
        else:
            cur = torch.cuda.current_stream()
            self._dp_stream.wait_stream(cur)
            with torch.cuda.stream(self._dp_stream):
                self._backward(8)
                self._allreduce(tlo, thi, False)
            self._backward(2)
            cur.wait_stream(self._dp_stream)          # explicit order: tail all-reduce complete before the head one is issued
            self._allreduce(hlo, hhi, False)
        self._update()

    def _step_body(self, after_forward=None, at_recurrence=None):
        """One whole step as straight-line stream code - the unit a single hipGraph holds (one process, or data-parallel
        with captured collectives)."""
        if self.dp:
            self._dp_step_body(after_forward, at_recurrence)
        else:
            self._fwd_bwd(after_forward, at_recurrence)
            self._update()

    @property
    def single_graph(self):
        """True when run() replays ONE graph per step (what features.WaveformFrontEnd can fold the next batch's features into)."""
        return self.use_graph and (not self.dp or self.dp_capture)

    # ---- public ------------------------------------------------------------------------------------
    def load_batch(self, x, x_ema, target):
        self.invalidate_batch()
        self.x.copy_(x.reshape(self.x.shape), non_blocking=True)
        if x_ema is not None:
            self.x_ema.copy_(x_ema.reshape(self.x.shape), non_blocking=True)
        self.target.copy_(target, non_blocking=True)

    def run(self):
        """One step on the batch currently in self.x / self.x_ema / self.target."""
        if self._p2p is not None and self._p2p.poll():
            # (a pinned host word the kernel raises: no synchronisation.  The launch that timed out has already NaN-filled its
            # gradients; this stops the run at the next step instead of letting it train on)
            raise _lib.SedError(f"peer all-reduce: {self._p2p.poll()} cross-rank waits ran out of their budget (a rank did not "
                                "launch the same sequence of collectives, died, or fell further behind than SED_P2P_TIMEOUT_S); "
                                "the gradients of that step were filled with NaN")
        # which form of the step: forwards that find their patch moments in ctx (valid: the previous run left them there) and / or
        # a tail that computes them for the next run (the batch is resident: nothing was loaded since the previous run)
        key = (self._mom_valid, self._resident and self.moments_ahead)
        self._mom_ready, self._mom_next = key
        graph = self.use_graph and self._warm >= 2
        if graph:
            gs = self._graph_sets.get(key)
            if gs is None:
                mode = (self.dp_capture, self.dp_schedule)
                self._graph_a = self._graph_w = self._graph_c = self._graph_b = None
                self._capture()
                if (self.dp_capture, self.dp_schedule) != mode:       # a capture fell back to another schedule: for every form
                    self._graph_sets = {}
                gs = self._graph_sets[key] = (self._graph_a, self._graph_w, self._graph_c, self._graph_b)
            self._graph_a, self._graph_w, self._graph_c, self._graph_b = gs
        if not self.dp:
            if graph:
                self._graph_a.replay()
            else:
                self._fwd_bwd()
                self._update()
        elif self.dp_capture:
            self._graph_a.replay() if graph else self._dp_step_body()
        else:
            self._dp_step_eager_collectives(graph)
        self._warm += 1
        self.steps_done += 1
        self._mom_valid = self._mom_next       # (the tail computed them for the batch that is in self.x now)
        self._resident = True
        self._mom_ready = self._mom_next = False

    def step(self, x, x_ema, target):
        """``x_ema`` is ignored (may be None) in supervised mode."""
        self.load_batch(x, x_ema, target)
        self.run()

    def _capture(self):
        torch.cuda.synchronize(self.device)
        cap = dict(stream=self._cap_stream)
        if self.dp:
            cap["capture_error_mode"] = "thread_local"      # see _collective_capture_works
        if self.dp and not self.dp_capture:
            overlap = self.dp_schedule == "overlap" and not self.cnn_frozen
            ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga, **cap):
                self._fwd_bwd()
            if overlap:
                gw, gc = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(gw, **cap):
                    self._backward(8)
                with torch.cuda.graph(gc, **cap):
                    self._backward(2)
                self._graph_w, self._graph_c = gw, gc
            with torch.cuda.graph(gb, **cap):
                self._update()
            self._graph_a, self._graph_b = ga, gb
        elif self.dp:
            # collectives captured into the step's graph.  Every rank must end up with the same schedule: if the capture
            # fails anywhere, all ranks fall back to "single" with an eager collective between two graph segments.
            import torch.distributed as dist
            ok = 1.0
            try:
                ga = torch.cuda.CUDAGraph()
                with torch.cuda.graph(ga, **cap):
                    self._dp_step_body()
            except Exception as e:                     # noqa: BLE001 - anything the capture raises means "not capturable here"
                ok, ga = 0.0, None
                self._capture_error = repr(e)
            flag = torch.tensor([ok], device=self.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.pg)
            if flag.item() == 1.0:
                self._graph_a = ga
            else:
                self.dp_capture, self.dp_schedule = False, "single"
                torch.cuda.synchronize(self.device)
                self._capture()
        else:
            ga = torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga, **cap):
                self._fwd_bwd()
                self._update()
            self._graph_a = ga
        # capture executes nothing: the captured work runs on replay

    def meters(self, reduce=False):
        """The meters main.train logs (main.py:106-149); ONE device->host copy.  They are rank-local (each rank's share
        of the batch); ``reduce=True`` averages them over the process group - equal shares, so this is the meter of the
        global batch."""
        m = self.losses[:8].clone()
        if reduce and self.pg is not None and self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(m, op=dist.ReduceOp.SUM, group=self.pg)
            m /= self.world
        return dict(zip(LOSS_NAMES, m.tolist()))

    def rendezvous(self):
        """Host-side barrier of the data-parallel ranks + a device synchronise.  The in-kernel waits of the peer all-reduce tolerate
        SED_P2P_TIMEOUT_S (default 600 s) of skew between ranks, as a blocking collective would; call this after rank-asymmetric
        work that may take longer (a long validation on rank 0 only), so that no rank's GPU sits in a spinning kernel meanwhile.
        It is NOT triggered from a local clock inside run(): a rank that was delayed and one that was not would disagree on
        whether to enter the barrier, and the late one would wait for ever."""
        torch.cuda.synchronize(self.device)
        if self.pg is not None and self.world > 1:
            import torch.distributed as dist
            dist.barrier(group=self.pg)

    def check_health(self):
        """Raise if a cross-workgroup wait of the wide model's cluster recurrence (csrc/ggru.hip) ever timed out: the
        kernels then carried on with a stale hidden state and every result since is suspect.  The counter is sticky (only
        sed_crnn_buffers_init clears it); one 4-byte device->host copy per model.  train() calls this whenever it reads
        the meters."""
        if self._p2p is not None:
            n = self._p2p.errors()
            if n:
                raise _lib.SedError(f"peer all-reduce: {n} cross-rank waits timed out (a rank did not launch the same "
                                    "sequence of collectives, or died); gradients since then are invalid")
        if self._err_view is None:
            return
        off, nb = self._err_view
        for name, ctx in (("student", self.ctx_s), ("teacher", self.ctx_t)):
            if ctx.numel():
                n = int(ctx[off:off + 4].view(torch.int32).item())
                if n:
                    raise _lib.SedError(f"cluster GRU recurrence: {n} cross-workgroup waits timed out in the {name} model "
                                        "(the four workgroups of a chain were not co-resident); results are invalid")

    def read_state(self):
        raw = bytes(self.state.cpu().numpy().tobytes())
        return _lib.SedStepState.from_buffer_copy(raw)

    # ---- checkpoint / true resume (the reference can save but not resume, main.py:293-354) -------
    def optimizer_state_dict(self):
        """The Adam state in torch.optim.Adam's own state_dict layout (what main.py:302-305 stores under
        state['optimizer']['state_dict']), so the checkpoint stays loadable by stock torch."""
        st = self.read_state()
        params = list(self.student.parameters())
        state = {}
        for i, ((o0, o1, shp), _) in enumerate(zip(self.student._layout, params)):
            state[i] = {"step": torch.tensor(float(st.opt_step - 1)),
                        "exp_avg": self.exp_avg[o0:o1].reshape(shp).detach().cpu().clone(),
                        "exp_avg_sq": self.exp_avg_sq[o0:o1].reshape(shp).detach().cpu().clone()}
        group = {"lr": st.lr, "betas": (st.beta1, st.beta2), "eps": st.eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(params)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        for i, (o0, o1, _) in enumerate(self.student._layout):
            if i in sd["state"]:
                self.exp_avg[o0:o1].copy_(sd["state"][i]["exp_avg"].reshape(-1))
                self.exp_avg_sq[o0:o1].copy_(sd["state"][i]["exp_avg_sq"].reshape(-1))

    def state_dict(self):
        """Everything a bit-exact resume needs: both models in the reference's nested checkpoint layout (plus the
        attention layer it drops, CRNN.py:49-53), the Adam moments, and the device step state (step counters - hence
        the ramp-up, EMA alpha, bias corrections - and the dropout / noise seed chain)."""
        return {"format": 1,
                "model": {k: {n: t.detach().cpu().clone() for n, t in v.items()} for k, v in self.student.state_dict().items()},
                "model_ema": ({k: {n: t.detach().cpu().clone() for n, t in v.items()}
                               for k, v in self.teacher.state_dict().items()} if self.teacher is not None else None),
                "optimizer": self.optimizer_state_dict(),
                "step_state": bytes(self.state.cpu().numpy().tobytes()),
                "seed_user": self.seed_user,
                "steps_done": self.steps_done}

    def load_state_dict(self, sd):
        assert sd.get("format") == 1, "unknown checkpoint format"
        self.invalidate_batch()
        self.student.load(parameters=sd["model"])
        if self.teacher is not None and sd.get("model_ema") is not None:
            self.teacher.load(parameters=sd["model_ema"])
        self.student.flatten_parameters_(self.device)
        if self.teacher is not None:
            self.teacher.flatten_parameters_(self.device)
        self.load_optimizer_state_dict(sd["optimizer"])
        raw = np.frombuffer(sd["step_state"], dtype=np.uint8).copy()
        assert raw.size == self.state.numel(), "step state size mismatch"
        self.state.copy_(torch.from_numpy(raw))
        self.seed_user = int(sd.get("seed_user", self.seed_user))
        self.steps_done = int(sd.get("steps_done", 0))
        self._gs_offset = int(_lib.SedStepState.from_buffer_copy(bytes(sd["step_state"])).global_step) - self.steps_done
        if self.rank != 0:       # the file holds rank 0's stream; every other rank re-folds its own rank into the seed
            _lib.check(self.l.sed_step_state_update(_lib.ptr(self.state), self._folded_seed(), 0.0, 1, _lib.stream_ptr()),
                       "sed_step_state_update")
        torch.cuda.synchronize(self.device)

    def save_checkpoint(self, path, extra=None):
        self.check_health()            # never write parameters that a timed-out collective or recurrence has touched
        torch.save(dict(self.state_dict(), **(extra or {})), path)

    def load_checkpoint(self, path):
        sd = torch.load(path, map_location="cpu", weights_only=False)
        self.load_state_dict(sd)
        return sd


def _check_loss(m):
    loss = m["loss"]
    assert not (loss != loss or loss > 1e5), 'Loss explosion: {}'.format(loss)       # main.py:147
    assert not loss < 0, 'Loss problem, cannot be negative'                            # main.py:148


def _epoch_start(step_obj, pg0, epoch, n_batches):
    step_obj.set_lr(pg0["lr"])        # an lr the caller changed between epochs is honoured (utils.py:227-241)
    # main.py:74: global_step = epoch * len(train_loader) + i - recomputed from `epoch` at every call.  A call sequence
    # epoch = 0, 1, 2 ... over one loader finds the device counter already there; a fresh step object entered with
    # epoch = k (a resumed run that did not load_checkpoint), a repeated or a skipped epoch gets the reference's value
    if step_obj.global_step_host != int(epoch) * n_batches:
        step_obj.set_global_step(int(epoch) * n_batches)


def _epoch_end(step_obj, epoch, start, log):
    m = step_obj.meters()
    _check_loss(m)
    step_obj.check_health()
    log('Epoch: {}\tTime {:.2f}\t{}'.format(epoch, time.time() - start,
                                            "\t".join(f"{k} {v:.4g}" for k, v in m.items())))
    return m


def _train_resident(rset, model, optimizer, epoch, ema_model, weak_mask, strong_mask, n_epoch, log, check_every):
    """train() over a ResidentFeatureSet: one fe.run() per step, no host batch.  The front-end's batch sequence runs on across
    calls (batch 0 of the next epoch is gathered during this epoch's last step); ``epoch`` sets global_step as in train()."""
    from .resident import ResidentFrontEnd
    start = time.time()
    n_batches = len(rset)
    pg0 = optimizer.param_groups[0]
    # with a process group the step works on this rank's share of each batch: main.py's global masks become dist.local_masks
    weak_mask, strong_mask = rset.step_masks(weak_mask, strong_mask)
    step_obj = getattr(model, "_mt_step", None)
    if step_obj is not None and rset.process_group is not None:
        B = step_obj.B
        have = (step_obj.wlo, step_obj.whi, step_obj.slo, step_obj.shi)
        want = (_slice_range(weak_mask, B) if weak_mask is not None else (0, 0)) + \
               (_slice_range(strong_mask, B) if strong_mask is not None else (0, 0))
        if have != want:
            raise ValueError(f"the model's step was built with masks {have} (weak lo, hi, strong lo, hi); this rank's share of the "
                             f"set needs {want}")
    if step_obj is None:
        model.to(rset.device)
        if ema_model is not None:
            ema_model.to(rset.device)
        step_obj = MeanTeacherStep(model, ema_model, rset.batch, rset.frames, n_batches * n_epoch // 2, weak_mask, strong_mask,
                                   lr=pg0["lr"], betas=pg0["betas"], eps=pg0["eps"], process_group=rset.process_group)
        model._mt_step = step_obj
    fe = getattr(model, "_mt_frontend", None)
    if fe is None or fe.rs is not rset or fe.step is not step_obj:
        # (a front-end built in a resumed run starts its augmentation draws at this epoch, not again at epoch 0's rows)
        fe = model._mt_frontend = ResidentFrontEnd(step_obj, rset)
        fe.aug_epoch = int(epoch)                      # (nothing is drawn before the first run())
    _epoch_start(step_obj, pg0, epoch, n_batches)
    for i in range(n_batches):
        fe.run()
        if (i + 1) % check_every == 0:
            _check_loss(step_obj.meters())
            step_obj.check_health()
    return _epoch_end(step_obj, epoch, start, log)


def train(train_loader, model, optimizer, epoch, ema_model=None, weak_mask=None, strong_mask=None, n_epoch=100,
          log=print, check_every=50):
    """main.train (main.py:52-165) with the loop body replaced by MeanTeacherStep.  With ``ema_model=None`` and
    two-element batches ``(batch_input, target)`` it is main_simple_CRNN.train (main_simple_CRNN.py:31-82).

    ``optimizer`` supplies lr / betas / eps (its per-tensor state is not used: Adam moments live in the
    step object's flat buffers, kept on ``model._mt_step`` across epochs).

    ``train_loader`` may also be a ``resident.ResidentFeatureSet``: the epoch's batches are then gathered from HBM one
    batch ahead inside the step's hipGraph (``resident.ResidentFrontEnd``, kept on ``model._mt_frontend`` across epochs) -
    same meters, loss checks, log line and global_step."""
    from .resident import ResidentFeatureSet
    if isinstance(train_loader, ResidentFeatureSet):
        return _train_resident(train_loader, model, optimizer, epoch, ema_model, weak_mask, strong_mask, n_epoch, log,
                               check_every)
    start = time.time()
    step_obj = getattr(model, "_mt_step", None)
    it = iter(train_loader)
    n_batches = len(train_loader)
    pg0 = optimizer.param_groups[0]

    for i in range(n_batches):
        batch = next(it)
        if ema_model is None:
            (batch_input, target), ema_batch_input = batch, None
        else:
            batch_input, ema_batch_input, target = batch
        if step_obj is None:
            B, T = batch_input.shape[0], batch_input.shape[-2]
            dev = torch.device("cuda", torch.cuda.current_device())
            model.to(dev)
            if ema_model is not None:
                ema_model.to(dev)
            step_obj = MeanTeacherStep(model, ema_model, B, T, n_batches * n_epoch // 2, weak_mask, strong_mask,
                                       lr=pg0["lr"], betas=pg0["betas"], eps=pg0["eps"])
            model._mt_step = step_obj
        if i == 0:
            _epoch_start(step_obj, pg0, epoch, n_batches)
        step_obj.step(batch_input.to(step_obj.device, non_blocking=True),
                      ema_batch_input.to(step_obj.device, non_blocking=True) if ema_batch_input is not None else None,
                      target.to(step_obj.device, non_blocking=True))
        # the reference asserts on the loss after EVERY batch (main.py:147-148), which costs it a host sync per step;
        # here the meters are read back every `check_every` steps and after the last one
        if (i + 1) % check_every == 0:
            _check_loss(step_obj.meters())
            step_obj.check_health()
    return _epoch_end(step_obj, epoch, start, log)


# ---- training on recording-level tags ------------------------------------------------------------------------------------------
def recording_tag_batches(n_windows, max_windows, seed, epoch):
    """The batches of one ``train_recording_tags`` epoch: ``n_windows`` [n_rec] windows per recording ->
    ``(runs, order)``.  ``runs``: ``longrec.recording_tag_runs`` - runs of consecutive recordings covering ``0 .. n_rec`` once,
    packed greedily within ``max_windows`` windows (a recording with more raises ``ValueError``); ``order``: the permutation
    of the runs drawn by ``np.random.default_rng([seed, epoch])``, the order the epoch visits them in."""
    from .longrec import recording_tag_runs
    runs = recording_tag_runs(n_windows, max_windows)
    return runs, _tag_batch_order(len(runs), seed, epoch)


def _tag_batch_order(n_batches, seed, epoch):
    return np.random.default_rng([int(seed), int(epoch)]).permutation(n_batches)


def _tags_loss(long_set, model, run, tables, targets, known=None, spans=None, weighting="taper", pieces=None):
    """The loss of one batch of either level - the recordings ``run = (r0, r1)`` of ``long_set`` - with its graph: the run's
    windows through the set's eval gather, ``model(x, return_attention=True)``, the pooled tags (``inference._pooled``), the
    BCE.  ``tables = (k, at, rec_win0, rec_frame0)``: ``tag_batches``' tables.  ``spans`` None: one row per recording, the
    plain mean ``binary_cross_entropy`` against ``targets[r0:r1]``.  ``spans = (span3, rec_span0 of every run rebased and
    concatenated like the tables, the set's span offsets on the host, the runs' known-pair counts)``: the rows are the run's
    spans, the BCE weighted by ``known`` and scaled by pairs / known pairs (a host number).  ``pieces``: the dict of
    ``LongRecordingSet.span_tag_batches`` - the batch is then its batch ``k`` (``run`` is not used), pieces of recordings with
    their own tables and ``rec_span_off``, pooled by the piece entries.  Returns ``(loss, err)``; nothing synchronises."""
    from .inference import _pooled
    k, at, win0_all, frame0_all = tables
    if pieces is None:
        r0, r1 = run
        w0, w1 = int(long_set.rec_win0_host[r0]), int(long_set.rec_win0_host[r1])
        frames_host = long_set.rec_frame0_host[r0:r1 + 1] - long_set.rec_frame0_host[r0]
        g0, g1, span = r0, r1, None
    else:
        _, frames_host, span0_local, off_host = pieces["tables"][k]
        w0, g0 = pieces["win"][k][0], pieces["rows"][k][0]
        w1, g1 = w0 + pieces["win"][k][1], g0 + pieces["rows"][k][1]
    if spans is not None and pieces is not None:
        span3, span0_all, _, counts = spans
        span = (span3, frames_host, (span0_local, span0_all[at[k]:at[k + 1]]),
                (off_host, pieces["rec_span_off"][at[k]:at[k + 1] - 1]))
    elif spans is not None:
        span3, span0_all, span0_host, counts = spans
        g0, g1 = int(span0_host[r0]), int(span0_host[r1])
        span = (span3, frames_host, (span0_host[r0:r1 + 1] - g0, span0_all[at[k]:at[k + 1]]))
    x = long_set.eval_batch(w0, w1 - w0)
    strong, _, att = model(x, return_attention=True)
    tags, err, _ = _pooled("pooled_tags" if spans is None else "pooled_span_tags", strong, att, win0_all[at[k]:at[k + 1]],
                           frame0_all[at[k]:at[k + 1]], int(frames_host[-1]), long_set.hop3, weighting, w1 - w0, span)
    target = targets[g0:g1]
    if spans is None:
        return torch.nn.functional.binary_cross_entropy(tags, target), err
    loss = torch.nn.functional.binary_cross_entropy(tags, target, weight=known[g0:g1])
    return loss * (target.numel() / int(counts[k])), err


def _tags_epoch(who, label, long_set, targets, known, counts, spans, model, optimizer, epoch, ema_model, max_windows, seed, log,
                pieces=None):
    """The one epoch on pooled tags, behind ``train_recording_tags`` and ``train_span_tags`` (``who``, for the messages;
    ``label``: the loss's name in the log line).  ``targets`` [rows, nclass]: host floats, one row per recording or per span;
    ``known`` / ``counts`` / ``spans = (span3, the set's span offsets on the host)``: ``span_tag_plan``'s mask, known-pair
    counts and span table, or None at the recording level - every run is then visited.  A run with a count of 0 is skipped:
    no forward, no optimizer or EMA step, though it keeps its place ``i`` in the order.  ``pieces``: the dict of
    ``LongRecordingSet.span_tag_batches`` (``train_span_tags(split_long=True)``) - its batches take the place of the runs, the
    rest of the epoch is the same.  Returns the mean loss over the runs that ran."""
    dev = long_set.device
    if pieces is None:
        runs, at, win0_all, frame0_all = long_set.tag_batches(max_windows)
    else:
        runs, at, win0_all, frame0_all = pieces["batches"], pieces["at"], pieces["rec_win0"], pieces["rec_frame0"]
    order = _tag_batch_order(len(runs), seed, epoch)
    start = time.time()
    if pieces is not None:
        spans, known = (spans[0], pieces["rec_span0"], spans[1], counts), torch.from_numpy(known).to(dev)
    elif spans is not None:
        span3, span0_host = spans
        span0_all = torch.from_numpy(np.concatenate([span0_host[r0:r1 + 1] - span0_host[r0] for r0, r1 in runs])).to(dev)
        spans, known = (span3, span0_all, span0_host, counts), torch.from_numpy(known).to(dev)
    targets = torch.as_tensor(targets, dtype=torch.float32).to(dev)
    model.to(dev)
    model.train()
    n_batches, n_ran = len(runs), 0
    loss_sum = torch.zeros((), dtype=torch.float32, device=dev)
    err_all = torch.zeros(1, dtype=torch.int32, device=dev)
    for i, k in enumerate(order):
        if counts is not None and counts[k] == 0:
            continue
        optimizer.zero_grad()
        loss, err = _tags_loss(long_set, model, runs[k], (int(k), at, win0_all, frame0_all), targets, known, spans, pieces=pieces)
        loss.backward()
        optimizer.step()
        if ema_model is not None:
            update_ema_variables(model, ema_model, 0.999, int(epoch) * n_batches + i)
        loss_sum += loss.detach()
        err_all |= err
        n_ran += 1
    mean = float(loss_sum.item()) / n_ran
    bits = int(err_all.item())
    if bits:
        raise _lib.SedError(f"{who}: the pooling kernels raised error bits {bits} (16: malformed tables, 32: a "
                            "recording its windows do not cover)")
    assert not (mean != mean or mean > 1e5), 'Loss explosion: {}'.format(mean)
    if log is not None:
        log('Epoch: {}\tTime {:.2f}\t{} {:.4g}'.format(epoch, time.time() - start, label, mean))
    return mean


def recording_tags_loss(long_set, tags_dev, model, run, tables, weighting="taper"):
    """The loss of one ``train_recording_tags`` batch - the recordings ``run = (r0, r1)`` of ``long_set`` - with its graph:
    the run's windows through the set's eval gather, ``model(x, return_attention=True)``, ``inference.pooled_tags``, the mean
    ``binary_cross_entropy`` over the run's (recording, class) pairs.  Returns ``(loss, err)``."""
    return _tags_loss(long_set, model, run, tables, tags_dev, weighting=weighting)


def train_recording_tags(long_set, tags, model, optimizer, epoch, ema_model=None, max_windows=64, seed=0, log=None):
    """One epoch of training on RECORDING-LEVEL tags: ``long_set`` a ``LongRecordingSet`` (recordings of any lengths, as
    overlapping windows), ``tags`` [n_rec, nclass] float targets in [0, 1] - all the labels a weakly labelled recording has.
    A window's own ``weak`` cannot be held to the recording's tags (the event may sit in another window), so the loss is on
    the tag pooled over the whole blended timeline (``inference.pooled_tags``); its gradient reaches every window of the
    recording through the posteriors and the attention (``sed_stitch_weak_backward``, ``sed_crnn_backward_att``).

    A batch is a run of consecutive recordings of at most ``max_windows`` windows (``LongRecordingSet.tag_batches``; a recording
    with more raises ``ValueError``), the batch order is drawn from (``seed``, ``epoch``).  Per batch: forward in train mode,
    mean BCE over the batch's (recording, class) pairs, ``backward()``, ``optimizer.step()`` (a torch optimizer over
    ``model.parameters()``), and with ``ema_model`` ``update_ema_variables(model, ema_model, 0.999, epoch * n_batches + i)`` as
    ``train()`` counts steps.  Nothing synchronises inside the epoch: the kernels' error word is read once at its end
    (nonzero raises ``SedError``), with the mean loss, which is returned."""
    from .longrec import LongRecordingSet
    if not isinstance(long_set, LongRecordingSet):
        raise ValueError("train_recording_tags needs a LongRecordingSet")
    tags_np = tags.detach().cpu().numpy() if torch.is_tensor(tags) else np.asarray(tags)
    if tags_np.ndim != 2 or tags_np.shape[0] != long_set.n_rec:
        raise ValueError(f"tags must be [n_rec = {long_set.n_rec}, nclass], got {tags_np.shape}")
    if not ((tags_np >= 0) & (tags_np <= 1)).all():
        raise ValueError("tags must lie in [0, 1]")
    return _tags_epoch("train_recording_tags", "recording_tag_loss", long_set, tags_np, None, None, None, model, optimizer, epoch,
                       ema_model, max_windows, seed, log)


# ---- training on span-level tags -----------------------------------------------------------------------------------------------
def span_tag_plan(rec_win0_host, rec_frame0_host, span_tags, max_windows, span3, split_long=False, T3=None, hop3=None):
    """The host-side plan of one ``train_span_tags`` epoch, nothing touches a GPU: the runs of ``recording_tag_runs``, the span
    table of the whole set and, per run, the count of KNOWN (span, class) pairs - a NaN target is unknown.  Returns a dict:
    ``runs``, ``rec_span0`` (host int64 [n_rec + 1]), ``total_spans``, ``span3`` (clamped as ``inference.span_table`` clamps
    it), ``targets`` float32 [total_spans, nclass] (the NaNs replaced by 0), ``known`` float32 (1 where the target is known),
    ``counts`` int64 [n_runs] and ``ran`` (the runs with at least one known pair: the others are skipped, no forward and no
    optimizer step).  ValueError for targets of another shape than the span table's or outside [0, 1].

    ``split_long=True`` (it needs the windows' geometry ``T3`` / ``hop3`` in label frames): a recording with more than
    ``max_windows`` windows does not raise but is cut into PIECES (``longrec.span_pieces``) - runs of consecutive spans with
    exactly the windows that cover them, one batch each.  ``runs`` is then the list of batches (lists of
    ``longrec.SpanPiece``), ``counts`` / ``ran`` are per batch, and two more keys say what the cut costs: boundary windows of
    neighbouring pieces cover spans of both and are forwarded in BOTH batches, ``forwarded_windows`` is the number of windows
    an epoch forwards and ``forwarded`` its ratio to the set's windows (1.0 without a long recording)."""
    from .inference import span_table
    from .longrec import recording_tag_runs, span_piece_tables, span_pieces
    rec_win0_host, rec_frame0_host = np.asarray(rec_win0_host, dtype=np.int64), np.asarray(rec_frame0_host, dtype=np.int64)
    rec_span0, _, total_spans, span3 = span_table(np.diff(rec_frame0_host), span3)
    tags_np = span_tags.detach().cpu().numpy() if torch.is_tensor(span_tags) else np.asarray(span_tags)
    if tags_np.ndim != 2 or tags_np.shape[0] != total_spans:
        raise ValueError(f"span_tags must be [total_spans = {total_spans}, nclass] for spans of {span3} label frames, got "
                         f"{tags_np.shape}")
    known = ~np.isnan(tags_np)
    if not ((tags_np[known] >= 0) & (tags_np[known] <= 1)).all():
        raise ValueError("span_tags must lie in [0, 1] (NaN: unknown)")
    extra = {}
    if split_long:
        if T3 is None or hop3 is None:
            raise ValueError("split_long needs T3 and hop3, the windows' length and hop in label frames")
        runs = span_pieces(np.diff(rec_win0_host), np.diff(rec_frame0_host), T3, hop3, span3, max_windows)
        tables = [span_piece_tables(b, rec_win0_host, rec_span0) for b in runs]
        counts = np.asarray([int(known[t[6]:t[6] + t[7]].sum()) for t in tables], dtype=np.int64)
        forwarded = int(sum(t[5] for t in tables))
        extra = {"forwarded_windows": forwarded, "forwarded": forwarded / float(rec_win0_host[-1] - rec_win0_host[0])}
    else:
        runs = recording_tag_runs(np.diff(rec_win0_host), max_windows)
        counts = np.asarray([int(known[rec_span0[r0]:rec_span0[r1]].sum()) for r0, r1 in runs], dtype=np.int64)
    return {"runs": runs, "rec_span0": rec_span0, "total_spans": total_spans, "span3": span3,
            "targets": np.where(known, tags_np, 0).astype(np.float32), "known": known.astype(np.float32), "counts": counts,
            "ran": [k for k in range(len(runs)) if counts[k] > 0], **extra}


def span_tags_loss(long_set, span_tags_dev, known_dev, model, run, tables, span3, weighting="taper"):
    """The loss of one ``train_span_tags`` batch - the recordings ``run = (r0, r1)`` of ``long_set`` - with its graph: the run's
    windows through the set's eval gather, ``model(x, return_attention=True)``, ``inference.pooled_span_tags``, then the
    ``binary_cross_entropy`` summed over the run's KNOWN (span, class) pairs and divided by their count.  ``span_tags_dev`` /
    ``known_dev`` [total_spans of the set, nclass] float32: the targets (0 where unknown) and the 0 / 1 mask of the known
    pairs; ``tables = (k, at, rec_win0, rec_frame0, rec_span0, rec_span0_host, counts)``: ``tag_batches``' tables, the runs'
    rebased span tables concatenated the same way, the set's span offsets and the runs' known-pair counts on the host.
    The sum is taken as the masked mean over all the run's pairs times pairs / known (a host number): with every pair known
    that is ``recording_tags_loss``'s mean BCE operation for operation.  Returns ``(loss, err)``; nothing synchronises."""
    return _tags_loss(long_set, model, run, tables[:4], span_tags_dev, known_dev, (span3,) + tuple(tables[4:]), weighting)


def train_span_tags(long_set, span_tags, model, optimizer, epoch, tag_span=None, span3=None, ema_model=None, max_windows=64,
                    seed=0, log=None, split_long=False):
    """One epoch of training on SPAN-LEVEL tags: ``train_recording_tags`` with one target vector per span of every recording
    instead of one per recording - a long recording assembled from weakly labelled clips, or coarse annotations of an hour
    of audio.  ``span_tags`` [total_spans, nclass] floats in [0, 1], the rows in ``inference.span_table(long_set, span3)``'s
    order (its total must match, ``ValueError`` otherwise); a NaN target is "unknown" and that (span, class) pair takes no
    part.  Exactly one of ``tag_span`` (seconds, rounded down to label frames by ``inference.tag_span_frames``) and
    ``span3`` (label frames) gives the span length; it is clamped to the longest recording.

    The loss is on ``inference.pooled_span_tags``: its gradient reaches the windows through ``sed_stitch_span_tags_backward``
    and ``sed_crnn_backward_att``, localised to the span - a class absent from a span pushes that span's posteriors down.
    The epoch is ``train_recording_tags``'s own (one loop serves both): batches, their order from (``seed``, ``epoch``), the
    optimizer and EMA steps (``epoch * n_batches + i``, ``i`` the batch's place in that order) and the end-of-epoch checks; a
    batch without a known pair is skipped (no forward, no optimizer or EMA step - the host knows from the targets).  Per batch
    the BCE is summed over its known pairs and divided by their count.  Nothing synchronises inside the epoch: the masks,
    counts and span tables are prepared once at its start, the kernels' error word is read once at its end (nonzero raises
    ``SedError``), with the mean loss over the batches that ran, which is returned.  A recording with more than
    ``max_windows`` windows raises ``ValueError`` - unless ``split_long=True``.

    ``split_long=True``: a span's tag depends only on the windows that cover the span, so such a recording is trained in
    PIECES (``longrec.span_pieces``, ``LongRecordingSet.span_tag_batches``): runs of consecutive spans with exactly the windows
    that cover them, as many spans as fit in ``max_windows`` windows, one batch per piece; shorter recordings are batched as
    before.  A piece's tags are bit-equal to the whole recording's on the same window posteriors and its gradient is that of
    exactly its own spans' loss terms (``sed_stitch_piece_span_tags`` and its backward) - nothing is cut on the host and no
    blend changes.  The price: boundary windows of neighbouring pieces cover spans of both, so they are forwarded in BOTH
    batches (``span_tag_plan(..., split_long=True)["forwarded"]`` is the ratio of forwarded windows to windows); and a model
    in train mode sees each piece as a batch of its own (dropout masks and batch statistics are per batch, as for any two
    batches).  The epoch is the same loop over the plan's batches.  A span that alone needs more than ``max_windows`` windows
    raises ``ValueError``.  Recording-level tags (``train_recording_tags``) still need a recording in one forward."""
    from .inference import _Cfg, tag_span_frames
    from .longrec import LongRecordingSet
    if not isinstance(long_set, LongRecordingSet):
        raise ValueError("train_span_tags needs a LongRecordingSet")
    if (tag_span is None) == (span3 is None):
        raise ValueError("give exactly one of tag_span (seconds) and span3 (label frames)")
    if span3 is None:
        span3 = tag_span_frames(tag_span, long_set.pooling_time_ratio * _Cfg.hop_length / _Cfg.sample_rate)
    plan = span_tag_plan(long_set.rec_win0_host, long_set.rec_frame0_host, span_tags, max_windows, span3, bool(split_long),
                         long_set.T3, long_set.hop3)
    if not plan["ran"]:
        raise ValueError("span_tags has no known target: every entry is NaN")
    pieces = None
    if split_long:
        pieces = long_set.span_tag_batches(max_windows, plan["span3"])
        assert pieces["batches"] == plan["runs"]
    else:
        assert long_set.tag_batches(max_windows)[0] == plan["runs"]
    return _tags_epoch("train_span_tags", "span_tag_loss", long_set, plan["targets"], plan["known"], plan["counts"],
                       (plan["span3"], plan["rec_span0"]), model, optimizer, epoch, ema_model, max_windows, seed, log, pieces)
