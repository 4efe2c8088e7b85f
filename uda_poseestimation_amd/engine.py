"""Mean-teacher training step of the reference (train_human.py:244-302 `pretrain`, :305-458 `train`) on the MI355X path.

The reference keeps this logic inside its train scripts; this harness reproduces the order of operations so that
bench.py, smoke() and the tests can drive the hot path the way `train_human.py` does:

    zero_grad -> [style s2t / t2s] -> teacher forward (no grad, train-mode BN) -> re-warp teacher heat-maps
    -> [occlusion] -> student(x_s), student(x_t_stu) (two separate forwards) -> re-warp student heat-maps
    -> JointsMSE(source) -> activations / rectify / k-th value mask -> ConsLoss -> backward
    -> (data parallel: one all-reduce of the flat gradient buffer over RCCL) -> Adam -> EMA -> PCK

Data parallelism: one process per GPU, the batch is sharded per image, every rank holds full
student / teacher replicas; the only collectives are the gradient all-reduce (student only) and a tiny all-gather of
the per-key-point confidences so that the mask threshold stays the GLOBAL-batch k-th value.  BN statistics stay per
rank, as with the reference's nn.DataParallel.
"""
import contextlib
import numpy as np
import os

import torch
import torch.distributed as dist

from . import adversarial
from . import data_gpu
from . import ops
from . import optim as fused_optim
from . import utils as mt
from . import warp
from .lib import keypoint_detection as kd
from .lib.models.loss import ConsLoss, JointsMSELoss

_INPUTS = ("x_s", "label_s", "weight_s", "x_t_stu", "x_t_tea")      # the batch tensors of a step, in call order


def _dist_on():
    # UDAPOSE_FORCE_DIST=1 (test hook): a one-rank process group still takes the data-parallel path, so the real RCCL
    # collectives and the three-graph step can be exercised on a one-GPU box
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or os.environ.get("UDAPOSE_FORCE_DIST", "0") == "1"


class GradSync:
    """All-reduce (mean) of the student's flat fp32 gradient buffer over RCCL/xGMI.  (The PoseResNet executor writes every
    parameter gradient into views of a single buffer.)  Either ONE collective per step (`sync()`), or two buckets so that
    the first - the suffix holding layer3 / layer4 / upsampling / head, 94 % of the bytes, final when backward part 1 has
    run - travels under backward part 2: `start_upper()` right after part 1, `finish()` after part 2."""

    def __init__(self, model, comm_dtype="fp32"):
        self.model = model
        self.reset()
        # 'bf16': the buckets travel in bf16 (udapose_comm_*: one rounding per contribution, all-to-all of shards, fp32 accumulation on
        # the shard's owner, the MEAN rounded to bf16 once more for the all-gather of the averaged shards): half the bytes per xGMI
        # link, two bf16 roundings per averaged gradient element.  RCCL backend only.
        self.comm_dtype = comm_dtype
        self._cbuf = {}
        # timing (bench.py): HIP events around finish() on the current stream = what the step WAITS for communication
        self.profile = False
        self._events = []

    def reset(self):
        # an exchange in flight: the Work of the suffix's collective, its view, the bf16 exchange's side stream (an aborted capture)
        self._work, self._upper, self._cstream = None, None, None

    def _flat(self):
        flat = getattr(self.model, "_flat_grad", None)
        if flat is None:
            raise RuntimeError("GradSync: model has no flat gradient buffer yet (run backward first)")
        return flat

    def _reduce_bf16(self, t, tag):
        """Average the fp32 bucket `t` over the ranks with bf16 on the wire (synchronous with respect to the current stream)."""
        from ._hip import check, lib, ptr, stream
        if dist.get_backend() != "nccl":
            raise RuntimeError("GradSync(comm_dtype='bf16') needs the RCCL backend")
        w, n = dist.get_world_size(), t.numel()
        m = (n + w - 1) // w
        m = (m + 7) // 8 * 8
        buf = self._cbuf.get(tag)
        if buf is None or buf[0].numel() != w * m or buf[0].device != t.device:
            buf = (torch.empty(w * m, dtype=torch.bfloat16, device=t.device), torch.empty(w * m, dtype=torch.bfloat16, device=t.device),
                   torch.empty(m, dtype=torch.bfloat16, device=t.device))
            self._cbuf[tag] = buf
        send, recv, mine = buf
        check(lib().udapose_comm_pack_bf16(stream(), ptr(t), n, ptr(send), w * m), "comm_pack_bf16")
        dist.all_to_all_single(recv, send)
        check(lib().udapose_comm_shard_mean(stream(), ptr(recv), w, m, ptr(mine)), "comm_shard_mean")
        dist.all_gather_into_tensor(send, mine)
        check(lib().udapose_comm_unpack_bf16(stream(), ptr(send), ptr(t), n), "comm_unpack_bf16")

    def _reduce(self, t, async_op=False, tag="all"):
        if self.comm_dtype == "bf16":
            self._reduce_bf16(t, tag)
            return None
        if dist.get_backend() == "nccl":
            return dist.all_reduce(t, op=dist.ReduceOp.AVG, async_op=async_op)   # RCCL averages in the collective: no second sweep
        w = dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=async_op)          # gloo (CPU tests, shared-GPU test) has no AVG
        if not async_op:
            t.mul_(1.0 / dist.get_world_size())
        return w

    def __call__(self):
        if not _dist_on():
            return
        ev = self._tick()
        self._reduce(self._flat())
        self._tock(ev)

    def _tick(self):
        if not self.profile:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _tock(self, e0):
        if e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self._events.append((e0, e1))

    def exposed_ms(self):
        """Mean time per step the compute stream spent inside the communication calls (after a synchronize)."""
        if not self._events:
            return None
        v = [a.elapsed_time(b) for a, b in self._events]
        self._events = []
        return sum(v) / len(v)

    def start_upper(self):
        """Launch the all-reduce of the gradient suffix on the communicator's own stream (it waits for what is enqueued on the
        current stream - backward part 1 and the sum of the two passes - and then runs beside whatever comes next)."""
        if not _dist_on():
            return
        flat = self._flat()
        self._upper = flat[self.model.grad_split_offset():]
        if self.comm_dtype == "bf16":
            # a side stream runs the bf16 exchange of the suffix beside backward part 2 (the collectives' own streams wait for it)
            if getattr(self, "_cstream", None) is None:
                self._cstream = torch.cuda.Stream(device=flat.device)
            cur = torch.cuda.current_stream()
            self._cstream.wait_stream(cur)
            with torch.cuda.stream(self._cstream):
                self._reduce_bf16(self._upper, "upper")
            self._work = "stream"
            return
        self._work = self._reduce(self._upper, async_op=True, tag="upper")

    def finish(self):
        """All-reduce the prefix (layer2 / layer1 / stem: 6 % of the bytes), then join the suffix's collective."""
        if not _dist_on():
            return
        flat = self._flat()
        ev = self._tick()
        self._reduce(flat[:self.model.grad_split_offset()], tag="lower")
        if self._work == "stream":
            torch.cuda.current_stream().wait_stream(self._cstream)
            self._work = None
        elif self._work is not None:
            self._work.wait()                        # the current stream waits for the suffix's collective
            if dist.get_backend() != "nccl":
                self._upper.mul_(1.0 / dist.get_world_size())
            self._work = None
        self._tock(ev)


def pick_concurrent_streams(device, n=3, candidates=10):
    """`n` torch streams whose kernels demonstrably run side by side.  HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4)
    by a least-users rule that depends on every stream the process has created so far, and two streams on one queue
    serialise (tools/probe_stream_pairs.py: with 4 queues a third of all pairs do).  So the choice is MEASURED: a short spin kernel on each
    stream of a pair, started together - wall time ~T: concurrent, ~2T: same queue - over `candidates` fresh streams until `n` mutually
    concurrent ones are found (falls back to the first `n` if there is no such set).  ~50 ms, once, at capture time."""
    import itertools
    import time
    pool = [torch.cuda.Stream(device=device) for _ in range(candidates)]
    cycles = 400_000

    def wall(ss):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for s_ in ss:
            with torch.cuda.stream(s_):
                torch.cuda._sleep(cycles)
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0

    wall(pool[:1])
    t1 = min(wall(pool[:1]) for _ in range(3))
    ok = {}
    for i, j in itertools.combinations(range(candidates), 2):
        ok[(i, j)] = min(wall([pool[i], pool[j]]) for _ in range(2)) < 1.5 * t1
    for comb in itertools.combinations(range(candidates), n):
        if all(ok[p_] for p_ in itertools.combinations(comb, 2)):
            return [pool[i] for i in comb], True
    return pool[:n], False


def gather_activates(act):
    """All ranks' [N_local, K] confidences -> flat global vector (for the global-batch k-th value, train_human.py:429)."""
    if not _dist_on():
        return None
    bufs = [torch.empty_like(act) for _ in range(dist.get_world_size())]
    dist.all_gather(bufs, act.contiguous())
    return torch.cat([b.reshape(-1) for b in bufs])


class _StyleAdapter:
    """The three call forms of a style net behind two operations: a batch is SUMMARISED once per step, from its original images, and every
    transfer is made from two summaries.  FDA (lib.models.fda.FDANet: spectrum / transfer): the low-frequency spectrum.  AdaIN (Style_net.Net:
    encode_features / transfer_from_features): relu4_1 - the reference's two style_net(...) calls encode each batch twice; same kernels, same
    inputs, same bits.  Plain (the reference's call, style_net(content, style, alpha, clamp=)[2]): the image itself.
    ASYMMETRY, kept: the eager step takes the plain call for an AdaIN net whose compute_losses is set; a captured step, whose summaries
    live in static buffers, ignores that flag and refuses a net that offers neither fast protocol."""

    def __init__(self, style_net, captured=False):
        self.style_net, self.captured = style_net, captured
        net = self.net = getattr(style_net, "module", style_net)          # (a single-device DataParallel wrap, as in the reference)
        self.kind, self.keys = "plain", None           # (keys: the static buffers of a captured step's summaries)
        if hasattr(net, "spectrum") and hasattr(net, "transfer"):
            self.kind, self.keys = "fda", ("sp_s", "sp_t")
        elif hasattr(net, "encode_features") and hasattr(net, "transfer_from_features"):
            self.kind, self.keys = "adain", ("f_s", "f_t")
        elif captured:
            raise TypeError(f"GraphedTrainStep: style_net {type(net).__name__} offers neither spectrum() / transfer() nor encode_features() / "
                            "transfer_from_features(); a captured style pass needs one of the two protocols")

    @property
    def form(self):
        if self.kind == "adain" and not self.captured and getattr(self.net, "compute_losses", False):
            return "plain"
        return self.kind

    def summarize(self, img, out=None):
        if self.form == "fda":
            return self.net.spectrum(img, out=out)
        if self.form == "plain":
            return img
        f = self.net.encode_features(img)
        return f if out is None else out.copy_(f)

    def transfer(self, content_img, sum_content, sum_style, alpha, clamp, out=None):
        if self.form == "fda":
            return self.net.transfer(content_img, sum_content, sum_style, alpha, clamp=clamp, out=out)
        if self.form == "plain":
            g = self.style_net(sum_content, sum_style, alpha, clamp=clamp)[2]
        else:
            g = self.net.transfer_from_features(sum_content, sum_style, alpha, clamp=clamp)
        return g if out is None else out.copy_(g)


class MeanTeacherTrainer:
    def __init__(self, student, teacher, lr=1e-4, teacher_alpha=0.999, lambda_c=1.0, mask_ratio=0.5, sigma=2, image_size=256,
                 heatmap_size=64, use_sgd=False, style_net=None, recover=None, s2t_freq=0.5, t2s_freq=0.5, s2t_alpha=(0.0, 1.0),
                 t2s_alpha=(0.0, 1.0), rng=None, occlude_rate=-1.0, occlude_thresh=0.9, occlude_size=10, image_px=None, precision=None,
                 loss_scale_init=65536.0, loss_scale_interval=2000, grad_comm="fp32", criterion=None, con_criterion=None, ent_criterion=None,
                 lambda_ent=0.0, params=None, warp_mode="nearest"):
        """params: what the student's optimizer is built from - an iterable of parameters or of group dicts, e.g.
        student.get_parameters(lr) (pose_resnet.py:572-577: the backbone at a tenth of the rate when finetune=True); None:
        student.parameters().  Group dicts carry their own lr; dynamic loss scaling needs a single group.
        warp_mode: "nearest" (the reference's) or "bilinear" - the interpolation of the two heat-map re-warps of a step: the teacher's
        views before their mean, and the student's y_t_stu_recon (under autograd).  The occlusion path's IMAGE warps stay nearest in either
        mode: they paste patches at integer boxes and are not under autograd."""
        if warp_mode not in warp.MODES:
            raise ValueError(f"warp_mode {warp_mode!r}: one of {warp.MODES}")
        self.warp_mode = warp_mode
        # a single-device nn.DataParallel wrap (the reference's call form) is unwrapped: the engine drives the executor's own entry points
        # (prepare / forward_deferred_bn / finish_wgrad ...), which live on the module
        student, teacher = getattr(student, "module", student), getattr(teacher, "module", teacher)
        self.student, self.teacher = student, teacher
        # the supervised and the consistency loss, called as the reference calls them (train_human.py:421,432): None = the scripts' own
        # JointsMSELoss / ConsLoss; any lib.models.loss class of the same call form may be given (JointsKLLoss, ConsSoftmaxLoss, ...).
        # ent_criterion (optional, e.g. EntLoss): lambda_ent * ent_criterion(student's re-warped target heat-maps) joins loss_all
        self.criterion = criterion if criterion is not None else JointsMSELoss()
        self.con_criterion = con_criterion if con_criterion is not None else ConsLoss()
        self.ent_criterion, self.lambda_ent = ent_criterion, lambda_ent
        # coral_criterion (optional, e.g. GramCoralLoss): lambda_coral * coral_criterion(y_s, y_t_stu) joins loss_all - the student's source
        # heat-maps against its OWN output on the target view BEFORE the re-warp (the re-warp zero-fills borders, and CORAL aligns output
        # statistics).  The covariances are over this rank's batch, like the BatchNorm statistics: no collective.  Both are ATTRIBUTES, set
        # after construction like the switches below (trainer.coral_criterion = GramCoralLoss(2); trainer.lambda_coral = 0.5) and before a
        # GraphedTrainStep is built from the trainer: the constructor's parameter list is pinned by tests/test_soft_argmax_cpu.py and
        # tests/test_warp_bilinear_cpu.py.
        self.coral_criterion, self.lambda_coral = None, 0.0
        # skeleton_prior (optional): {'mean', 'std'} [K,K] tables, e.g. utils.SkeletonPrior(K, device).finalize() over source labels.  When set,
        # the teacher's re-warped mean heat-map is replaced by generate_prior_map(prior, it, prior_gamma, prior_sigma, v3=prior_v3,
        # multiply=True) - the map times the structural prior of its own decoded joints (utils.py:111-145) - and everything downstream sees the
        # product: the occlusion picks, `activates`, the confidence mask, rectify.  Attributes like the two above, set before a GraphedTrainStep
        # is built.  Data parallel: the tables are the same on every rank; nothing is communicated.
        self.skeleton_prior, self.prior_gamma, self.prior_sigma, self.prior_v3 = None, 2, 2, False
        # mask_mode: how the teacher's confidences become the consistency mask (utils.confidence_mask) - "global", the reference's single
        # batch-wide k-th value; "per_joint", a k-th value per joint (the pool is all ranks' samples: the all-gather that exists); "threshold",
        # confidences above mask_threshold, a fixed or ramped absolute value (no collective).  Attributes like the ones above.  mask_mode is
        # baked into a captured step; mask_threshold lives in a device scalar that is refreshed outside the graph, beside
        # stu_optimizer.sync_hyper(), so a captured step follows a host change of it (a curriculum ramp).
        self.mask_mode, self.mask_threshold = "global", 0.5
        self._mask_thr = None               # [device scalar, the host value it holds]
        # adv_eps (None: off): the student's target view is replaced by its adversarial view (adversarial.adversarial_view) -
        # the view moved inside the adv_norm ("l2" / "linf") ball of radius adv_eps in the direction that increases the plain mean-squared
        # distance between the student's re-warped heat-maps and the teacher's re-warped mean map (times the skeleton prior where one is
        # set): the "strong view" of consistency training picked by gradient.  adv_steps (1 .. 4) probe passes of the student, none of which
        # leaves a trace on it; adv_step: the step of an iteration (None: adv_eps for one step, 2.5 * adv_eps / adv_steps otherwise).  It
        # runs after the occlusion, clamps to `recover`, and the rest of the step sees the perturbed view.  Attributes like the ones above;
        # on / off, adv_norm and adv_steps are baked into a captured step, adv_eps / adv_step live in device scalars refreshed outside the
        # graph (sync_adv).  Data parallel: the probes are per rank, before the split backward; nothing is communicated.
        self.adv_eps, self.adv_norm, self.adv_steps, self.adv_step = None, "l2", 1, None
        self._adv_dev = None                # [device scalars (eps, step), the host values they hold, the clamp on the device]
        # view_merge (None: off, the plain warp.mean_views): "mean" or "trimmed" - the k >= 2 re-warped teacher views are merged by agreement
        # (warp.merge_views): per (sample, joint) the views whose peak lies within view_radius heat-map pixels of the medoid
        # peak are the inliers; "trimmed" averages the inliers only, "mean" keeps the plain mean; either way a joint on which fewer than
        # view_min views (None: all k) are inliers is taken out of the consistency mask, in every mask_mode (the gate is confidence_mask's
        # tea_mask=).  The skeleton prior, the occlusion picks, `activates`, rectify and the adversarial probe see the merged map as they see
        # the mean.  The step's dict gains view_agree, view_n_inliers, view_spread2.  Attributes like the ones above; view_radius lives in a
        # device scalar refreshed outside any graph (sync_view_radius).  GraphedTrainStep stages k views when it is built with a list of them
        # and refuses a trainer with view_merge set only when built with a single view.  Data parallel: the views, their peaks and the gate
        # are per rank and per sample; nothing is communicated.
        self.view_merge, self.view_radius, self.view_min = None, 2.0, None
        self._view_rad = None               # [device scalar, the host value it holds]
        # scheduled: names out of SCHEDULABLE whose values the step - eager or captured - reads from DEVICE memory, so that
        # a captured step follows a ramp of them (utils.sigmoid_rampup, ema_alpha_warmup ...) instead of refusing the change: the loss weights
        # as 0-d fp32 tensors in loss_all, teacher_alpha as the fp32 pair (alpha, 1 - alpha) of the EMA sweeps, mask_ratio as the int32 k-th
        # index of the mask's select.  sync_schedule() uploads what changed, outside any capture; GraphedTrainStep.step calls it.  An
        # attribute like the ones above, set before a GraphedTrainStep is built and frozen afterwards; (): every launch is what it was.
        self.scheduled = ()
        self._sched, self._sched_pool = None, None      # [8 device words, the host bytes they hold] | the mask's pool size, once a step has seen it
        # precision: None keeps what the networks are set to (a new PoseResNet is 'auto': a differentiable forward outside
        # autocast runs bf16, the teacher's no-grad forward the fp32-grade 'f16x2' mode).
        # 'reference' = the reference's own precision mix (train_human.py:346-358,414): the student in fp16 (its autocast dtype)
        #   with GradScaler's dynamic loss scaling kept on the device (optim.py), the teacher and the style network OUTSIDE autocast
        #   in fp32 - here the fp32-grade 'f16x2' mode (three fp16 MFMAs per K step; heat-maps within ~4e-5 of the fp32 oracle).
        # 'strict' = the same mix with an fp32-grade student FORWARD (PoseResNet precision 'strict': the f16x2 forward, the fp16 backward
        #   under the same loss scaling - the gradients are not fp32-grade); teacher and style network as in 'reference'.
        # 'bf16' / 'fp16': student AND teacher in that 16-bit type (BASELINE.json's benched configuration is 'bf16'; the style
        #   network keeps its own setting).
        # ('reference_fp32': the 'reference' mix with the EXACT fp32 MFMA forms for the teacher and the style network - the slow way to the same
        # numbers, kept for A/B timing of the f16x2 mode)
        mixes = {"reference": ("fp16", "f16x2", "f16x2"), "reference_fp32": ("fp16", "fp32", "fp32"), "strict": ("strict", "f16x2", "f16x2")}
        self._style = _StyleAdapter(style_net) if style_net is not None else None       # (unwraps the style net)
        if precision is not None:
            student.precision, teacher.precision, style_precision = mixes.get(precision, (precision, precision, None))
            if style_precision is not None and self._style is not None and hasattr(self._style.net, "precision"):
                self._style.net.precision = style_precision
        # Loss scaling is decided ONCE, here, from what the student can run: 'fp16', or 'auto' (which resolves to fp16 whenever the step
        # runs under torch.autocast, the reference's call form) get the device-side GradScaler; a scaled bf16 step is exact (powers of
        # two), an unscaled fp16 step underflows silently - _check_scaler() refuses that combination at step time
        sp = getattr(student, "precision", "bf16")
        scaled = sp in ("fp16", "auto", "strict")       # ('strict': the fp16 backward)
        # the teacher's fp32-grade plans live in the student's library build, so the fused optimizer tail hands both plans to one .so
        if hasattr(teacher, "aux_lib_kind"):
            teacher.aux_lib_kind = "fp16" if sp in ("fp16", "strict") else "bf16"
        sc = dict(dynamic_loss_scale=True, init_scale=loss_scale_init, growth_interval=loss_scale_interval) if scaled else {}
        opt_params = params if params is not None else student.parameters()
        if use_sgd:
            self.stu_optimizer = fused_optim.FusedSGD(opt_params, lr=lr, momentum=0.9, weight_decay=1e-4, nesterov=True, **sc)
        else:
            self.stu_optimizer = fused_optim.FusedAdam(opt_params, lr=lr, **sc)
        self.tea_optimizer = mt.OldWeightEMA(teacher, student, alpha=teacher_alpha)   # ctor copies student -> teacher
        self.sync = GradSync(student, comm_dtype=grad_comm)
        self.lambda_c, self.mask_ratio, self.sigma = lambda_c, mask_ratio, sigma
        self.ratio = image_size / heatmap_size
        self.style_net, self.recover = style_net, recover
        self.s2t_freq, self.t2s_freq, self.s2t_alpha, self.t2s_alpha = s2t_freq, t2s_freq, s2t_alpha, t2s_alpha
        self.rng = rng if rng is not None else np.random   # the reference draws from the global np.random
        self._side = None
        self.fuse_rectify = True    # activates and the rectified teacher heat-maps from one arg-max sweep (False: two launches, the reference's two calls)
        self.concurrent = True      # False: run the three branches back to back on the current stream (profiling)
        # adaptive key-point occlusion (train_human.py:374-412); rate <= -1 disables it like `--occlude-rate -1`
        self.occlude_rate, self.occlude_thresh, self.occlude_size = occlude_rate, occlude_thresh, occlude_size
        self.image_px = image_px if image_px is not None else image_size
        # False: the reference's host draws in its order (rand / choice / randint x 2 per qualifying sample, after one read-back
        # of the confidences).  True: four uniform draws per sample go to the device and udapose_occlusion_pick takes the
        # decisions there - same distribution, no read-back, capturable (GraphedTrainStep needs it)
        self.device_occlusion = False
        self.occl_rng = self.rng            # generator of the host-side occlusion draws (the reference: the global np.random)
        self._occl = None                   # ("host", aug_param_stu) | ("device", theta_back [N,1,6], u [N,4])
        # mirrored views: the left / right joint pairs that un-mirroring a flagged sample's heat-maps swaps - a sequence of
        # pairs (possibly empty) or a key of lib.keypoint_detection.FLIP_PAIRS; None: a batch with a flipped sample is refused
        self.flip_pairs = None
        # data parallel: cut the backward after layer3 and all-reduce the finished 94 % of the gradient under the rest of it
        # (None: whenever a process group is active and the network has the layer3 boundary)
        self.overlap_allreduce = None
        self.fuse_tail = True               # Adam / SGD + EMA + weight packs in one sweep (optim.FusedAdam / FusedSGD.fused_tail_step)
        self.stream_priority = 0            # priority of the branch streams (and of a captured step's origin stream): -1 = high
        self.merge_wgrad = True             # one rank: both passes' grouped weight gradients in one launch (pose_resnet.finish_wgrad)
        self.single_graph = True            # one rank: the optimizer tail is captured into the step's graph (one launch per step)
        self.sum_grads_in_tail = True       # ... which also adds the two passes' gradient buffers (no separate axpy; one rank only)
        self.sum_splits_in_tail = False     # opt-in: the sweep also adds the partial tiles of the split weight-gradient reductions (udapose_net_wgrad_pair_defer):
                                            # no split-sum launch, no write + re-read of those sums - bit-identical, but measured SLOWER in the step (the
                                            # sweep's split blocks wait on ks dependent loads per row; profiles/tail_ab_runs.txt), so it stays off
        self.fused_last = False

    @property
    def max_grad_norm(self):
        """Clipping of the student's update by the global gradient norm (FusedAdam / FusedSGD.max_grad_norm): None = off, a positive float,
        or float('inf') to measure only (stu_optimizer.grad_norm() / clip_coef()).  An ATTRIBUTE forwarding to stu_optimizer, set after
        construction like coral_criterion and before a GraphedTrainStep is built: on / off changes the captured launches, the value does not
        (it lives on the device).  Data parallel: the norm is taken in _update(), behind GradSync.finish(), on the reduced gradient - every
        rank forms the same bits and no collective is added."""
        return getattr(self.stu_optimizer, "max_grad_norm", None)

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        self.stu_optimizer.max_grad_norm = v

    def sync_mask_threshold(self, device=None):
        """The device scalar that holds mask_threshold, uploaded when the host value changed (a stream-ordered 4-byte copy, like
        stu_optimizer.sync_hyper()); never inside a capture, whose launches read the scalar."""
        v = float(self.mask_threshold)
        if self._mask_thr is None or (device is not None and self._mask_thr[0].device != torch.device(device)):
            if device is None:
                device = next(self.student.parameters()).device
            self._mask_thr = [torch.tensor(v, dtype=torch.float32, device=device), v]
        elif v != self._mask_thr[1] and not torch.cuda.is_current_stream_capturing():
            self._mask_thr[0].copy_(torch.tensor(v, dtype=torch.float32), non_blocking=True)
            self._mask_thr[1] = v
        return self._mask_thr[0]

    def sync_view_radius(self, device=None):
        """The device scalar that holds view_radius, uploaded when the host value changed (a stream-ordered 4-byte copy, like
        sync_mask_threshold()); never inside a capture, whose launch reads the scalar."""
        v = float(self.view_radius)
        if self._view_rad is None or (device is not None and self._view_rad[0].device != torch.device(device)):
            if device is None:
                device = next(self.student.parameters()).device
            self._view_rad = [torch.tensor(v, dtype=torch.float32, device=device), v]
        elif v != self._view_rad[1] and not torch.cuda.is_current_stream_capturing():
            self._view_rad[0].copy_(torch.tensor(v, dtype=torch.float32), non_blocking=True)
            self._view_rad[1] = v
        return self._view_rad[0]

    SCHEDULABLE = ("lambda_c", "lambda_ent", "lambda_coral", "teacher_alpha", "mask_ratio")
    # the device words of sync_schedule(): fp32 [lambda_c, lambda_ent, lambda_coral, alpha, 1 - alpha], int32 [k], two spare
    _SCHED_SLOT = {"lambda_c": 0, "lambda_ent": 1, "lambda_coral": 2, "teacher_alpha": 3, "mask_ratio": 5}

    def _scheduled_names(self):
        names = tuple(getattr(self, "scheduled", ()) or ())
        if isinstance(getattr(self, "scheduled", ()), str):
            names = (self.scheduled,)
        bad = [n for n in names if n not in self.SCHEDULABLE]
        if bad:
            raise ValueError(f"trainer.scheduled = {names!r}: {bad} cannot be scheduled; the names are {self.SCHEDULABLE}")
        return names

    def _schedule_words(self, names):
        """The eight 32-bit words the device holds for the scheduled names (slots of the others stay zero): an fp32 array whose word 5 is k's int32."""
        w = np.zeros(8, dtype=np.float32)
        for n in ("lambda_c", "lambda_ent", "lambda_coral"):
            if n in names:
                w[self._SCHED_SLOT[n]] = float(getattr(self, n))
        if "teacher_alpha" in names:
            w[3], w[4] = mt.ema_pair(self.tea_optimizer.alpha)      # (OldWeightEMA.step's pair: 1 - alpha in double, each rounded to fp32 here)
        if "mask_ratio" in names and self.mask_mode != "threshold" and self._sched_pool is not None:
            # ("threshold" ignores mask_ratio; before the first step the pool's size is unknown: that step uploads k before its own launch)
            w.view(np.int32)[5] = mt.mask_kth_index(self.mask_ratio, self._sched_pool, self.mask_mode)
        return w

    def sync_schedule(self, device=None):
        """The device words that hold the values of trainer.scheduled, uploaded when a host value changed (one stream-ordered 32-byte copy,
        like sync_mask_threshold()); never inside a capture, whose launches read them.  -> None with nothing scheduled, else a dict of device
        views: 0-d fp32 'lambda_c' / 'lambda_ent' / 'lambda_coral', fp32 [2] 'teacher_alpha' = (alpha, 1 - alpha), int32 [1] 'mask_ratio' = k."""
        names = self._scheduled_names()
        if not names:
            if getattr(self.tea_optimizer, "alpha_dev", None) is not None:
                self.tea_optimizer.alpha_dev = None
            return None
        w = self._schedule_words(names)
        if self._sched is None or (device is not None and self._sched[0].device != torch.device(device)):
            if device is None:
                device = next(self.student.parameters()).device
            self._sched = [torch.from_numpy(w.copy()).to(device), w.tobytes()]
        elif w.tobytes() != self._sched[1] and not torch.cuda.is_current_stream_capturing():
            self._sched[0].copy_(torch.from_numpy(w.copy()), non_blocking=True)
            self._sched[1] = w.tobytes()
        d = self._sched[0]
        views = {n: d[self._SCHED_SLOT[n]] for n in ("lambda_c", "lambda_ent", "lambda_coral") if n in names}
        if "teacher_alpha" in names:
            views["teacher_alpha"] = d[3:5]
        if "mask_ratio" in names:
            views["mask_ratio"] = d.view(torch.int32)[5:6]
        self.tea_optimizer.alpha_dev = views.get("teacher_alpha")
        return views

    def _check_view_merge(self, k):
        """view_merge set: a mode warp.merge_views knows, and at least two teacher views to merge."""
        if self.view_merge is None:
            return
        if self.view_merge not in warp.MERGE_MODES:
            raise ValueError(f"trainer.view_merge = {self.view_merge!r}: None or one of {tuple(warp.MERGE_MODES)}")
        if k < 2:
            raise ValueError(f"trainer.view_merge = {self.view_merge!r} merges the teacher's views by their agreement and needs at least two "
                             f"of them per step, got {k} (pass a list of k >= 2 target views, or set trainer.view_merge = None)")

    def sync_adv(self, device=None):
        """The device scalars that hold adv_eps and the iterations' step, uploaded when a host value changed (stream-ordered 8-byte copy, like
        sync_mask_threshold()); never inside a capture, whose launches read them.  -> (eps, step or None: the kernel's one-step form)."""
        eps = float(self.adv_eps)
        steps = int(self.adv_steps)
        step = float(self.adv_step) if self.adv_step is not None else (eps if steps == 1 else 2.5 * eps / steps)
        if self._adv_dev is None or (device is not None and self._adv_dev[0].device != torch.device(device)):
            if device is None:
                device = next(self.student.parameters()).device
            clamp = None        # (`recover` on the device, made once: the view's clamp must not copy from the host inside a capture)
            if self.recover is not None:
                clamp = tuple(torch.as_tensor(v, dtype=torch.float32).detach().reshape(-1).to(device) for v in self.recover)
            self._adv_dev = [torch.tensor([eps, step], dtype=torch.float32, device=device), (eps, step), clamp]
        elif (eps, step) != self._adv_dev[1] and not torch.cuda.is_current_stream_capturing():
            self._adv_dev[0].copy_(torch.tensor([eps, step], dtype=torch.float32), non_blocking=True)
            self._adv_dev[1] = (eps, step)
        d = self._adv_dev[0]
        return d[0], (None if (steps == 1 and self.adv_step is None) else d[1])

    def _mirror_perm(self, mirrors, num_joints, device):
        """The joint permutation the step's mirrored re-warps take: None when no view carries a mirror tensor (the plain launches)."""
        if all(m is None for m in mirrors):
            return None
        if self.flip_pairs is None:
            raise ValueError("the batch has mirrored views (a flip entry in its aug_param) and trainer.flip_pairs is None: set it to the "
                             "left / right joint pairs (a sequence of pairs, possibly empty, or a key of FLIP_PAIRS)")
        return warp.mirror_perm(self.flip_pairs, num_joints, device)

    def _mirror_tensors(self, aug_params, n, device):
        """Per view: the flip flags of its aug_param on the device (uint8 [N]), None for a view without a flagged sample - whose warps are
        then exactly the un-mirrored launches.  ValueError, before anything is launched, for a flagged sample without flip_pairs."""
        flags = [warp.aug_mirror(ap, n) for ap in aug_params]
        flags = [f if f is not None and bool(f.any()) else None for f in flags]
        if self.flip_pairs is None and any(f is not None for f in flags):
            self._mirror_perm(flags, 0, device)
        return [f.to(device, non_blocking=True) if f is not None else None for f in flags]

    def _adversarial_part(self, x_t_stu, theta_stu, target, mirror=None, perm=None):
        """(on the student's target stream, behind the teacher branch) the adversarial view of x_t_stu against the teacher's pseudo-labels."""
        eps, step = self.sync_adv(x_t_stu.device)
        cons = ConsLoss()

        def probe_loss(y):      # no mask, no rectify: nothing is communicated, nothing moves out of _loss_backward_part
            return cons(warp.warp_chain(y, theta_stu, self.warp_mode, mirror, perm if mirror is not None else None), target)
        return adversarial.adversarial_view(self.student, x_t_stu, probe_loss, eps, norm=self.adv_norm, steps=self.adv_steps, step=step,
                                            clamp=self._adv_dev[2], grad_scale=self.stu_optimizer.loss_scale())

    def _check_scaler(self):
        """An fp16 student forward needs the loss scaler the optimizer was built with (or the caller's own GradScaler: then build the
        trainer's optimizer yourself)."""
        hd = getattr(getattr(self.student, "module", self.student), "_last_hd", None)
        if hd is not None and hd.precision in ("fp16", "strict") and getattr(self.stu_optimizer, "_scaler", None) is None:
            raise RuntimeError(f"the student ran in {hd.precision} (an fp16 backward) but the trainer's optimizer has no dynamic loss scaling: fp16 "
                               "heat-map gradients underflow without it - construct MeanTeacherTrainer with precision='fp16' / 'reference' / "
                               "'strict' / 'auto'")

    # ------------------------------------------------------------------ train_human.py:262-302
    def pretrain_step(self, x_s, label_s, weight_s, x_t=None):
        self.student.train()
        self.stu_optimizer.zero_grad()
        if self.style_net is not None and self.s2t_freq > self.rng.rand():
            a = self.rng.uniform(*self.s2t_alpha)
            x_s = self.style_net(x_s, x_t, a, clamp=self.recover)[2]
        y_s = self.student(x_s)
        loss = self.criterion(y_s, label_s, weight_s)
        self._check_scaler()
        overlap = self._overlap()
        self.student.split_backward = overlap
        self.stu_optimizer.scale_loss(loss).backward()          # (scaler.scale(loss).backward(), train_human.py:285; identity in bf16)
        self.student.split_backward = False
        if overlap:
            self.sync.start_upper()
        self._sync_grads()
        self.stu_optimizer.step()
        return {"loss_all": loss.detach(), "loss_s": loss.detach(), "y_s": y_s.detach()}

    # ------------------------------------------------------------------ train_human.py:326-444
    def train_step(self, x_s, label_s, weight_s, x_t_stu, x_t_teas, aug_param_stu, aug_params_tea, with_accuracy=False):
        """Eager step from the loader's collated batch (aug_param tuples as produced by the reference's transforms)."""
        if not isinstance(x_t_teas, (list, tuple)):
            x_t_teas, aug_params_tea = [x_t_teas], [aug_params_tea]
        self._check_view_merge(len(x_t_teas))
        n, dev = x_t_stu.shape[0], x_t_stu.device
        theta_stu = warp.recon_thetas(aug_param_stu, n, self.ratio, dev)
        thetas_tea = [warp.recon_thetas(ap, n, self.ratio, dev) for ap in aug_params_tea]
        mirror_stu, *mirrors_tea = self._mirror_tensors([aug_param_stu] + list(aug_params_tea), n, dev)
        x_s_in, x_t_teas_in = self._style_part(x_s, list(x_t_teas))
        self._occl = None
        if self.occlude_rate > -1:
            if self.device_occlusion:
                self._occl = ("device", warp.occlusion_back_thetas(aug_param_stu, n, self.ratio, dev), self.draw_occlusion_uniforms(n, dev))
            else:
                if _dist_on() and self.style_net is not None and self.occl_rng is self.rng:
                    raise RuntimeError("data parallel with style transfer: the host occlusion draws are data dependent in number and "
                                       "would take the ranks' common style decisions out of step - set trainer.device_occlusion = True "
                                       "or give the occlusion its own generator (trainer.occl_rng)")
                self._occl = ("host", aug_param_stu)
        # (a step without a flagged sample makes the call it always made)
        mirrors = (mirror_stu, mirrors_tea) if mirror_stu is not None or any(m is not None for m in mirrors_tea) else ()
        out = self._forward_backward(x_s_in, label_s, weight_s, x_t_stu, x_t_teas_in, theta_stu, thetas_tea, *mirrors)
        self._sync_grads()
        self._update()
        if with_accuracy:
            _, avg_acc, cnt, _ = kd.accuracy(out["y_s"], label_s)
            out["acc_s"], out["cnt_s"] = avg_acc, cnt
        return out

    def draw_style_decisions(self):
        """The step's host draws for the style pass, in the reference's order (train_human.py:345-358): rand, [uniform], rand,
        [uniform] -> (alpha_s2t | None, alpha_t2s | None)."""
        if self.style_net is None:
            return None, None
        a_s2t = self.rng.uniform(*self.s2t_alpha) if self.s2t_freq > self.rng.rand() else None
        a_t2s = self.rng.uniform(*self.t2s_alpha) if self.t2s_freq > self.rng.rand() else None
        return a_s2t, a_t2s

    def draw_occlusion_uniforms(self, n, device=None):
        """[n,4] uniform numbers for this rank's samples.  Data parallel: every rank draws the GLOBAL batch's numbers and keeps its
        slice - with equally seeded generators the ranks' host streams stay in step (the style decisions that follow are per
        step for the whole global batch, as in the reference's single process) and the samples' draws stay independent."""
        if _dist_on():
            w, r = dist.get_world_size(), dist.get_rank()
            u = np.asarray(self.rng.rand(w * n, 4), dtype=np.float32)[r * n:(r + 1) * n]
        else:
            u = np.asarray(self.rng.rand(n, 4), dtype=np.float32)
        u = torch.from_numpy(np.ascontiguousarray(u))
        return u.to(device, non_blocking=True) if device is not None else u

    def _style_part(self, x_s, x_t_teas):
        """Bidirectional style transfer of the step's inputs (train_human.py:345-358), both from the ORIGINAL images: each batch is
        summarised once (_StyleAdapter), and only the first teacher view when t2s was not drawn."""
        a_s2t, a_t2s = self.draw_style_decisions()
        if a_s2t is None and a_t2s is None:
            return x_s, x_t_teas
        style, out_s, out_ts = self._style, x_s, x_t_teas
        with torch.no_grad():
            sum_s = style.summarize(x_s)
            sum_ts = [style.summarize(x_t) for x_t in (x_t_teas if a_t2s is not None else x_t_teas[:1])]
            if a_s2t is not None:
                out_s = style.transfer(x_s, sum_s, sum_ts[0], a_s2t, self.recover)
            if a_t2s is not None:
                out_ts = [style.transfer(x_t, sum_t, sum_s, a_t2s, self.recover) for x_t, sum_t in zip(x_t_teas, sum_ts)]
        return out_s, out_ts

    def _forward_part(self, x_s, label_s, weight_s, x_t_stu, x_t_teas, theta_stu, thetas_tea, mirror_stu=None, mirrors_tea=None):
        """All forwards of the step after the style pass (no host reads unless the occlusion draws on the host: capturable
        in a hipGraph).  mirror_stu / mirrors_tea: per view None or its flip flags on the device (uint8 [N]): every warp of a view that
        has them takes its mirrored form (the heat-map re-warps with the joint permutation of trainer.flip_pairs, the occlusion's image
        warps without), and a view without them the launches it always took."""
        student, teacher = self.student, self.teacher
        student.train()
        teacher.train()                     # the teacher's BN uses batch statistics too (train_human.py:321)
        self.stu_optimizer.zero_grad()
        # Three independent branches run on three HIP streams and meet at the consistency loss: the teacher branch (forward
        # + re-warp), the student's target-domain forward (+ re-warp) and the student's source-domain forward.  Their kernels
        # interleave on the device (measured: two concurrent fwd+bwd passes take 22.3 ms instead of 28.6 ms back to back).
        # Autograd runs each backward on the stream of its forward, so the two backward passes overlap as well; each pass
        # owns its activation arena, scratch workspace and (second pass) gradient buffer.  BN running statistics of the
        # target-domain forward are applied after the join, in the reference's call order (x_s first, then x_t_stu).
        main = torch.cuda.current_stream()
        if self._side is None or self._side[0].device != x_s.device:
            pr = self.stream_priority
            self._side = (torch.cuda.Stream(device=x_s.device, priority=pr), torch.cuda.Stream(device=x_s.device, priority=pr))
        s_tea, s_stu = self._side if self.concurrent else (main, main)
        occl = self._occl if self.occlude_rate > -1 else None
        adv, adv_gnorm = self.adv_eps is not None, None
        self._check_view_merge(len(x_t_teas))
        mirrors_tea = list(mirrors_tea) if mirrors_tea is not None else [None] * len(x_t_teas)
        perm = self._mirror_perm([mirror_stu] + mirrors_tea, label_s.shape[1], x_s.device)
        view_rad = self.sync_view_radius(x_s.device) if self.view_merge is not None else None      # (on `main`, before the branches fork)
        merged = None
        student.prepare(x_s)               # bf16 weight packs refreshed on `main` before the branches fork
        with torch.no_grad():
            teacher.prepare(x_t_teas[0])
        s_tea.wait_stream(main)
        s_stu.wait_stream(main)
        with torch.cuda.stream(s_tea), torch.no_grad():
            y_t_teas = [teacher(x_t) for x_t in x_t_teas]
            recons = [warp.warp_chain(y, th, self.warp_mode, m, perm if m is not None else None)
                      for y, th, m in zip(y_t_teas, thetas_tea, mirrors_tea)]
            if self.view_merge is None:
                y_t_tea_recon = warp.mean_views(recons)      # (k teacher views, train_human.py:361-372: one launch; k = 1: the view itself)
                tea_out = [y_t_tea_recon]
            else:
                # the same launch slot: the views' mean (of the inliers in "trimmed" mode) plus the per-joint agreement gate of the mask
                merged = warp.merge_views(recons, view_rad, self.view_merge, self.view_min)
                y_t_tea_recon = merged.mean
                tea_out = [t for t in merged if t is not None]
            if self.skeleton_prior is not None:
                y_t_tea_raw = y_t_tea_recon
                y_t_tea_recon = mt.generate_prior_map(self.skeleton_prior, y_t_tea_raw, self.prior_gamma, self.prior_sigma, v3=self.prior_v3,
                                                      multiply=True)
                tea_out = tea_out + [y_t_tea_recon]
        if occl is not None or adv:
            # the occlusion (and the adversarial view) needs the teacher's re-warped heat-maps: the source-domain forward is issued first
            # (it runs under the teacher's), the target-domain branch waits for the teacher
            y_s = student(x_s)
            s_stu.wait_stream(s_tea)
            for t in y_t_teas + recons + tea_out:
                t.record_stream(s_stu)
        with torch.cuda.stream(s_stu):
            if occl is not None:
                with torch.no_grad():
                    if occl[0] == "device":
                        x_t_stu, self.occluded = warp.occlude_keypoints_device(x_t_stu, y_t_tea_recon, theta_stu, occl[1], occl[2], self.ratio,
                                                                               self.image_px, self.occlude_rate, self.occlude_thresh,
                                                                               self.occlude_size, mirror=mirror_stu)
                    else:   # (one small D2H of confidences, as in the reference)
                        x_t_stu, self.occluded = warp.occlude_keypoints(x_t_stu, y_t_tea_recon, occl[1], self.ratio, self.image_px,
                                                                        self.occlude_rate, self.occlude_thresh, self.occlude_size, self.occl_rng,
                                                                        mirror=mirror_stu)
            if adv:
                x_t_stu, adv_gnorm = self._adversarial_part(x_t_stu, theta_stu, y_t_tea_recon, mirror_stu, perm)
            y_t_stu = student.forward_deferred_bn(x_t_stu)     # separate forwards: separate BN statistics per domain
            y_t_stu_recon = warp.warp_chain(y_t_stu, theta_stu, self.warp_mode, mirror_stu, perm if mirror_stu is not None else None)
        if occl is None and not adv:
            y_s = student(x_s)
        main.wait_stream(s_stu)
        student.apply_deferred_bn()         # (x_s first, then x_t_stu: the reference's call order, train_human.py:414-417)
        for t in (y_t_stu, y_t_stu_recon, x_t_stu):
            t.record_stream(main)
        main.wait_stream(s_tea)
        for t in y_t_teas + recons + tea_out:
            t.record_stream(main)
        with torch.no_grad():
            # activates from the heat-maps BEFORE rectify (train_human.py:427); the rectified maps (:431) come out of the same arg-max sweep
            if self.fuse_rectify:
                activates, y_t_tea_rect = mt.activations_and_rectify(y_t_tea_recon, self.sigma)
            else:
                activates, y_t_tea_rect = mt.heatmap_activations(y_t_tea_recon), None
        st = {"y_s": y_s, "y_t_stu": y_t_stu, "y_t_stu_recon": y_t_stu_recon, "y_t_tea_recon": y_t_tea_recon, "activates": activates, "y_t_tea_rect": y_t_tea_rect,
              "label_s": label_s, "weight_s": weight_s, "main": main, "s_stu": s_stu}
        if self.skeleton_prior is not None:
            st["y_t_tea_raw"] = y_t_tea_raw
        if merged is not None:
            st["view_agree"], st["view_n_inliers"], st["view_spread2"] = merged.agree, merged.n_inliers, merged.spread2
        if adv:
            adv_gnorm.record_stream(main)
            st["x_t_stu_adv"], st["adv_gnorm"] = x_t_stu, adv_gnorm
        return st

    def _overlap(self):
        on = self.overlap_allreduce
        if on is None:
            on = _dist_on()
        return bool(on) and hasattr(self.student, "finish_backward")

    def _sync_grads(self):
        """What sits between backward and the optimizer: nothing on one rank; with overlap, backward part 2 under the first
        bucket's all-reduce, then the second bucket; otherwise one all-reduce of the whole buffer."""
        if self._overlap() and self.student._pending_lower:
            self._backward_lower()
            self.sync.finish()
        else:
            self.sync()

    def _backward_lower(self, grads_part=2):
        student = self.student
        main = torch.cuda.current_stream()
        streams = {id(p[5]): p[5] for p in student._pending_lower}
        for stv in streams.values():
            if stv is not main:
                stv.wait_stream(main)              # (fork: inside a capture the side stream joins the graph here)
        student.finish_backward()
        for stv in streams.values():
            if stv is not main:
                main.wait_stream(stv)
        student.finish_grads(part=grads_part)

    def _loss_backward_part(self, st, gathered_activates):
        """Losses and backward from the forward state; `gathered_activates` = all ranks' confidences (None on one rank).
        With overlap (data parallel) this is backward PART 1 of both passes, the sum of their gradient suffixes and the launch
        of that suffix's all-reduce; _sync_grads() runs part 2 and the rest."""
        student = self.student
        main, s_stu = st["main"], st["s_stu"]
        overlap = self._overlap()
        student.split_backward = bool(overlap)
        # one rank: the two passes' grouped weight gradients go out as ONE launch after both gradient chains (finish_wgrad)
        merge = (not overlap) and self.merge_wgrad and hasattr(student, "finish_wgrad")
        student.merge_wgrad = bool(merge)
        if getattr(self, "_metrics_cb", None) is not None:
            self._metrics_cb(st)                # (GraphedTrainStep: decode + PCK of the source batch on an idle side stream, under the backward)
        loss_s = self.criterion(st["y_s"], st["label_s"], st["weight_s"])
        self._check_scaler()
        sched = None
        if self.scheduled:
            # the mask's pool: every gathered confidence ("global"), the gathered samples ("per_joint") - sync_schedule turns mask_ratio into k with it
            pool = gathered_activates.numel() if gathered_activates is not None else st["activates"].numel()
            self._sched_pool = pool // st["activates"].shape[1] if self.mask_mode == "per_joint" else pool
            sched = self.sync_schedule(st["activates"].device)
        with torch.no_grad():
            # threshold = k-th value over the GLOBAL batch (all-gather of [N,K] floats when data parallel)
            thr_dev = self.sync_mask_threshold(st["activates"].device) if self.mask_mode == "threshold" else None
            # (a scheduled mask_ratio: the int32 k in device memory in place of the ratio; "threshold" ignores either)
            ratio = sched["mask_ratio"] if (sched and "mask_ratio" in sched and self.mask_mode != "threshold") else self.mask_ratio
            # (view_agree: the 0 / 1 agreement gate of the merged teacher views, absent with view_merge off)
            tea_mask, _, mask_thr = mt.confidence_mask(st["y_t_tea_recon"], ratio, st.get("view_agree"), gathered_activates,
                                                       st["activates"], mode=self.mask_mode, threshold=thr_dev)
            y_t_tea_rect = st["y_t_tea_rect"] if st.get("y_t_tea_rect") is not None else mt.rectify(st["y_t_tea_recon"], sigma=self.sigma)
        loss_c = self.con_criterion(st["y_t_stu_recon"], y_t_tea_rect, tea_mask=tea_mask)
        # (a scheduled weight: the 0-d fp32 device tensor in place of the Python float, which the product rounds to the same fp32 value)
        lam = {n: (sched[n] if sched and n in sched else getattr(self, n)) for n in ("lambda_c", "lambda_ent", "lambda_coral")}
        loss_all = loss_s + lam["lambda_c"] * loss_c
        loss_ent = None
        if self.ent_criterion is not None:
            loss_ent = self.ent_criterion(st["y_t_stu_recon"])
            loss_all = loss_all + lam["lambda_ent"] * loss_ent
        loss_coral = None
        if self.coral_criterion is not None:
            loss_coral = self.coral_criterion(st["y_s"], st["y_t_stu"])
            loss_all = loss_all + lam["lambda_coral"] * loss_coral
        self.stu_optimizer.scale_loss(loss_all).backward()      # (scaler.scale(loss_all).backward(), train_human.py:436; identity in bf16)
        if s_stu is not main:
            main.wait_stream(s_stu)             # the target-domain backward ran on its own stream
        student.split_backward = False
        if merge:
            student.merge_wgrad = False
            student.finish_wgrad(defer_sum=self._tail_sums_splits())
        if overlap:
            student.finish_grads(part=1)    # the suffix of both passes is final: sum it ...
            if not torch.cuda.is_current_stream_capturing() or getattr(self, "capture_comm", False):
                self.sync.start_upper()     # ... and send it off (a captured step issues the collective between its graphs, or captures it: capture_comm)
        elif student._pending_lower:
            self._backward_lower(grads_part=0)      # (overlap forced off after part 1 ran: finish the backward here)
        else:
            # adds the second pass's gradient buffer (no-op when both ran on one stream) - unless the fused optimizer tail will
            # read both buffers itself (one rank: nothing else looks at the gradients in between)
            student.finish_grads(defer=self._tail_sums_grads())
        # (the re-warped heat-maps of both networks are handed out for the parity tests and bench.py's measured parity: references only)
        out = {"loss_all": loss_all.detach(), "loss_s": loss_s.detach(), "loss_c": loss_c.detach(), "y_s": st["y_s"].detach(),
               "tea_mask": tea_mask, "y_t_tea_recon": st["y_t_tea_recon"], "y_t_stu_recon": st["y_t_stu_recon"].detach()}
        if self.mask_mode != "global":
            out["mask_thr"] = mask_thr          # ([K] per joint; 0-d, the trainer's device scalar, in "threshold" mode)
        if loss_ent is not None:
            out["loss_ent"] = loss_ent.detach()
        if loss_coral is not None:
            out["loss_coral"] = loss_coral.detach()
            out["y_t_stu"] = st["y_t_stu"].detach()      # (what the criterion saw beside y_s: the target heat-maps before the re-warp)
        if "view_agree" in st:
            out["view_agree"], out["view_n_inliers"], out["view_spread2"] = st["view_agree"], st["view_n_inliers"], st["view_spread2"]
        if "x_t_stu_adv" in st:
            out["x_t_stu_adv"], out["adv_gnorm"] = st["x_t_stu_adv"], st["adv_gnorm"]      # (the view the student saw; ||d probe loss / d x|| per sample)
        if "y_t_tea_raw" in st:
            # (y_t_tea_recon above IS the product: the teacher's map as the rest of the step saw it)
            out["prior_map"], out["y_t_tea_raw"] = st["y_t_tea_recon"], st["y_t_tea_raw"]
        return out

    def _forward_backward(self, x_s, label_s, weight_s, x_t_stu, x_t_teas, theta_stu, thetas_tea, mirror_stu=None, mirrors_tea=None):
        st = self._forward_part(x_s, label_s, weight_s, x_t_stu, x_t_teas, theta_stu, thetas_tea, mirror_stu, mirrors_tea)
        return self._loss_backward_part(st, gather_activates(st["activates"]))

    def _tail_sums_grads(self):
        return bool(self.fuse_tail and self.sum_grads_in_tail and not _dist_on() and hasattr(self.stu_optimizer, "fused_tail_step")
                    and hasattr(self.student, "pending_grad_sum"))

    def _tail_sums_splits(self):
        # (a loss scaler's inf / nan check reads the gradient tensors between the weight gradients and the sweep: the fp16 step keeps the launch)
        # (the sweep that adds the split sums has an Adam form only: FusedSGD.tail_takes_split_sums is False)
        # (clipping by global norm reads the gradient tensors in the same place, for the same reason)
        return bool(self.sum_splits_in_tail and self._tail_sums_grads() and getattr(self.stu_optimizer, "_scaler", None) is None
                    and getattr(self.stu_optimizer, "max_grad_norm", None) is None
                    and getattr(self.stu_optimizer, "tail_takes_split_sums", False))

    def _update(self):
        # the optimizer, the EMA and the next forwards' weight packs of both networks in ONE sweep when the layout allows ...
        fuse = self.fuse_tail and hasattr(self.stu_optimizer, "fused_tail_step")
        if self.scheduled or getattr(self.tea_optimizer, "alpha_dev", None) is not None:
            self.sync_schedule()            # (a scheduled teacher_alpha: the pair both EMA forms read; outside a capture only)
        self.fused_last = bool(fuse and self.stu_optimizer.fused_tail_step(self.student, self.teacher, self.tea_optimizer))
        if not self.fused_last:
            if hasattr(self.student, "finish_grads"):
                self.student.finish_grads()     # (a sum left to the fused tail that did not run)
            self.stu_optimizer.step()
            self.tea_optimizer.step()       # EMA after the optimizer step (train_human.py:437-438)


# How the flip test runs its two evaluation forwards: "batched" = one forward of the 2N batch [x; mirror(x)] that
# udapose_hflip_batch(keep_original=1) writes, "two" = model(x) and model(mirror(x)).  The folded evaluation forward has no cross-image
# term: the two forms give the same bits, image for image, and the 2N form is the faster one (it holds a plan of 2N images).
FLIP_FORWARD_FORM = "batched"


def _flip_forward(model, x, perm, shift_heatmap, decode):
    """Both evaluation forwards and the merge launch: (merged [N,K,H,W], preds, maxvals), the last two None without decode.  The merge
    writes over the plain forward's heat-maps (the executor hands out a fresh output tensor per forward)."""
    if model.training:
        raise RuntimeError("the flip test is an evaluation forward: call model.eval() first (train-mode BatchNorm would mix the two views)")
    with torch.no_grad():
        x = x.float().contiguous()
        N = x.shape[0]
        if FLIP_FORWARD_FORM == "batched":
            y2 = model(ops.hflip_batch(x, keep_original=True))
            y, yf = y2[:N], y2[N:]
        else:
            y, yf = model(x), model(ops.hflip_batch(x))
        return kd._flip_merge(y, yf, perm, shift_heatmap, decode, out=y)


def flip_forward(model, x, flip_pairs, shift_heatmap=False):
    """Flip-test heat-maps of an eval-mode model: (model(x) + flip_back(model(mirror(x)), flip_pairs, shift_heatmap)) * 0.5, the mirror
    image made by udapose_hflip_batch and flip-back, joint swap and average by one udapose_flip_merge launch.  flip_pairs: a sequence of
    left / right joint pairs or a key of lib.keypoint_detection.FLIP_PAIRS."""
    perm = kd._perm_device(flip_pairs, model.num_keypoints, x.device)
    return _flip_forward(model, x, perm, shift_heatmap, False)[0]


def validate(batches, model, criterion=None, decode="argmax"):
    """The reference's validate() (train_human.py:461-500) on the device: eval mode, no grad; per-key-point PCK@0.05
    averaged over the set with batch-size weights, entries of -1 (key point absent from a batch) ignored exactly like
    `AverageMeterList(ignore_val=-1)` (lib/meter.py:18-36,65-82), and the batch-size weighted mean loss.  `batches` yields
    (x, label, weight[, meta]).  Decode and PCK run on the device and are ACCUMULATED there: one read-back at the end
    instead of the reference's 2 x 8.4 MB device->host copy + sync per batch.  Returns (acc_per_keypoint list, mean_loss)
    (the caller applies its dataset's group_accuracy).  decode: how the predictions are decoded for the PCK, as in
    lib.keypoint_detection.accuracy ("argmax", "soft", "quarter", "dark" or a callable)."""
    criterion = criterion or JointsMSELoss()
    was_training = model.training
    model.eval()
    acc_sum = acc_cnt = loss_sum = None
    n_seen = 0
    with torch.no_grad():
        for batch in batches:
            x, label, weight = batch[0], batch[1], batch[2]
            dev = next(model.parameters()).device
            x, label, weight = x.to(dev, non_blocking=True), label.to(dev, non_blocking=True), weight.to(dev, non_blocking=True)
            y = model(x)
            loss = criterion(y, label, weight)
            acc, _, _ = kd.accuracy_device(y, label, decode=decode)
            n = x.shape[0]
            present = (acc != -1).to(torch.float32)
            if acc_sum is None:
                acc_sum, acc_cnt, loss_sum = torch.zeros_like(acc, dtype=torch.float64), torch.zeros_like(acc, dtype=torch.float64), \
                    torch.zeros((), dtype=torch.float64, device=dev)
            acc_sum += (acc * present).double() * n
            acc_cnt += present.double() * n
            loss_sum += loss.detach().double() * n
            n_seen += n
    if was_training:
        model.train()
    if acc_sum is None:
        return [], float("nan")
    avg = torch.where(acc_cnt > 0, acc_sum / acc_cnt.clamp(min=1), torch.zeros_like(acc_sum))     # AverageMeter.avg starts at 0
    out = torch.cat([avg, (loss_sum / max(n_seen, 1)).reshape(1)]).cpu().tolist()                 # the one read-back
    sat = mt.split_saturations(reset=True)          # (the evaluation forward runs the fp32-grade f16x2 mode under 'auto': its range is fp16's)
    if sat:
        import warnings
        warnings.warn(f"validate(): {sat} f16x2 stores saturated at |x| = 65504 (or were NaN) since the last check - activations outside fp16's "
                      "range; run the model with precision='fp32' (exact, slower) to rule the format out")
    return out[:-1], out[-1]


class _FlipTestModel(torch.nn.Module):
    """What validate_flip() hands to validate() as its model: a call returns flip_forward()'s merged heat-maps and keeps the decode that came
    out of the merge launch, which `decoded` gives back as validate()'s decode callable."""

    def __init__(self, model, flip_pairs, shift_heatmap, decode):
        super().__init__()
        self.model, self.flip_pairs, self.shift_heatmap, self.decode = model, flip_pairs, shift_heatmap, decode
        self._last = None
        self.train(model.training)      # (validate() restores the mode it finds: the wrapped model's)

    def forward(self, x):
        perm = kd._perm_device(self.flip_pairs, self.model.num_keypoints, x.device)
        merged, preds, maxv = _flip_forward(self.model, x, perm, self.shift_heatmap, self.decode)
        self._last = (merged.data_ptr(), preds, maxv)
        return merged

    def decoded(self, heatmaps):
        if self._last is None or self._last[0] != heatmaps.data_ptr():
            raise RuntimeError("the merge launch's decode belongs to the heat-maps of the last flip-test forward")
        return self._last[1], self._last[2]


def validate_flip(batches, model, flip_pairs, criterion=None, decode="argmax", shift_heatmap=False):
    """validate() with the flip test (the reference's -f/--flip, train_animal.py:556): loss and PCK of flip_forward()'s merged heat-maps.
    flip_pairs: a sequence of left / right joint pairs or a key of lib.keypoint_detection.FLIP_PAIRS; shift_heatmap: Simple Baselines'
    one-pixel shift of the flipped output.  With decode="argmax" the predictions are the ones the merge launch decoded as it wrote; "soft",
    "quarter", "dark" or a callable decode the merged map as in validate().  validate() itself is unchanged: this hands it a model that runs the flip test."""
    kd.flip_perm(flip_pairs, model.num_keypoints)       # (a bad table fails here, before any forward)
    fused = isinstance(decode, str) and decode == "argmax"
    flipped = _FlipTestModel(model, flip_pairs, shift_heatmap, fused)
    return validate(batches, flipped, criterion, decode=flipped.decoded if fused else decode)


def evaluate(batches, model, thresholds=kd.PCK_THRESHOLDS, groups=None, criterion=None, decode="argmax", flip_pairs=None, shift_heatmap=False,
             norm=None, pixel_scale=1.0):
    """validate()'s loop (eval mode, no grad, the mode restored, the saturation warning) with a lib.keypoint_detection.PCKMeter in place of
    the per-batch PCK: the report of the whole set - PCK at every threshold of a curve, its AUC, the end-point error, joint groups - from
    integer counts kept on the device, so the numbers do not depend on how the set is cut into batches (validate()'s batch-weighted mean of
    per-batch fractions does: DESIGN.md 4.18) and nothing is read back before the end.  `batches` yields (x, label, weight[, meta]); a meta
    that is a dict with "target_coords" ([B,K,2] in heat-map pixels; optionally "visible" [B,K]) is scored against those instead of the
    label's arg-max.  thresholds: in the unit of `accuracy`'s thr (0.5 is PCK@0.05).  groups: a key of JOINT_GROUPS or a mapping, what the
    reference's dataset.group_accuracy(acc.average()) prints.  decode: as in validate().  flip_pairs: given, the forward is
    flip_forward's (shift_heatmap as there), and with decode="argmax" the merge launch's own decode is scored.  norm: None or a callable
    batch -> [B] device tensor of per-sample lengths in heat-map pixels.  Returns PCKMeter.report()'s dict plus "loss" (the batch-size
    weighted mean, as validate()) and "n" (the samples seen)."""
    criterion = criterion or JointsMSELoss()
    dev = next(model.parameters()).device
    meter = kd.PCKMeter(model.num_keypoints, thresholds, device=dev)      # (bad thresholds fail here, before any forward)
    if groups is not None:
        kd._joint_groups(groups)
    run = model
    if flip_pairs is not None:
        kd.flip_perm(flip_pairs, model.num_keypoints)
        fused = isinstance(decode, str) and decode == "argmax"
        run = _FlipTestModel(model, flip_pairs, shift_heatmap, fused)
        if fused:
            decode = run.decoded
    was_training = run.training
    run.eval()
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    n_seen = 0
    with torch.no_grad():
        for batch in batches:
            x, label, weight = batch[0], batch[1], batch[2]
            x, label, weight = x.to(dev, non_blocking=True), label.to(dev, non_blocking=True), weight.to(dev, non_blocking=True)
            meta = batch[3] if len(batch) > 3 and isinstance(batch[3], dict) and "target_coords" in batch[3] else None
            y = run(x)
            loss = criterion(y, label, weight)
            length = norm(batch) if norm is not None else None
            if meta is not None:
                vis = meta.get("visible")
                meter.update(y, decode=decode, target_coords=meta["target_coords"].to(dev), visible=None if vis is None else vis.to(dev),
                             norm=length)
            else:
                meter.update(y, label, decode=decode, norm=length)
            n = x.shape[0]
            loss_sum += loss.detach().double() * n
            n_seen += n
    if was_training:
        run.train()
    # the one read-back: the counts and the mean loss's bits in one int64 copy
    mean_loss = (loss_sum / max(n_seen, 1)) if n_seen else torch.full_like(loss_sum, float("nan"))
    packed = torch.cat([meter.state().reshape(-1), mean_loss.reshape(1).view(torch.int64)]).cpu()
    rep = kd.PCKMeter.report(packed[:-1].reshape(meter.state().shape), meter.thresholds, groups, pixel_scale)
    rep["loss"], rep["n"] = float(packed[-1:].view(torch.float64)), n_seen
    sat = mt.split_saturations(reset=True)          # (as validate(): the evaluation forward runs the f16x2 mode under 'auto')
    if sat:
        import warnings
        warnings.warn(f"evaluate(): {sat} f16x2 stores saturated at |x| = 65504 (or were NaN) since the last check - activations outside fp16's "
                      "range; run the model with precision='fp32' (exact, slower) to rule the format out")
    return rep


def predict(frames_u8, boxes, model, frame_idx=None, flip_pairs=None, shift_heatmap=False, decode="argmax", batch=32, input_size=None,
            mean=data_gpu.IMAGENET_MEAN, std=data_gpu.IMAGENET_STD, return_heatmaps=False, box_scores=None, nms=None):
    """Top-down inference on the device: pictures and boxes in, key points in the pictures' own pixels out.
    frames_u8 [F,Hs,Ws,3] uint8 CUDA; boxes [M,5] = (cx, cy, bw, bh, rot_deg) in pixels of their frames (lib.keypoint_detection.
    boxes_from_keypoints / boxes_from_center_scale make them) - a numpy array or a list, checked on the host (ValueError naming a bad
    row, before any launch), or a CUDA tensor, which is not read here; frame_idx [M]: the frame of every box (None: box m is on frame m).
    Per chunk of `batch` boxes: data_gpu's box crop to input_size (S or (H, W); None: 256, the reference's --image-size) normalised by
    mean / std, the evaluation forward, the decode ("argmax", "soft", "quarter", "dark" or a callable, as in validate()) and
    udapose_coords_to_image.  The last chunk is padded to `batch` with repeats of its first box and the padding rows are dropped: the
    folded evaluation forward has no cross-image term, so one plan serves every chunk and the result does not depend on `batch`.
    flip_pairs (a sequence of left / right joint pairs or a key of lib.keypoint_detection.FLIP_PAIRS; shift_heatmap as in flip_forward):
    the flip test - the crop launch writes the mirrored crops behind the plain ones, one forward of 2 x batch images, udapose_flip_merge;
    with decode="argmax" the merge launch's own decode is used.
    Returns {"keypoints": [M,K,2] fp32 (x, y) in pixels of the frames, "confidence": [M,K] the (merged) map's maximum, "status": [M] uint8,
    1 = the box was refused (its key points mean nothing), "heatmaps": [M,K,Hh,Wh] with return_heatmaps}, all on the device.  Eval mode
    under no_grad, the model's mode restored.  Nothing is read back and, with device boxes, nothing is uploaded: a call can be captured
    into a graph, and a replay follows new values in the same boxes tensor.  Outside a capture the call ends with validate()'s
    saturation check of the f16x2 evaluation forward (the one host synchronisation, after the last launch).
    nms: None - one pose per box, as above, and exactly those launches; True or a dict of lib.keypoint_detection.oks_nms's
    keyword arguments (sigmas, oks_thr, vis_thr, want_matrix) - the poses are rescored (box_scores [M]: the detector's scores, a CUDA
    tensor or host numbers; None: 1) and thinned per frame by greedy OKS-NMS on the device, with the boxes' areas, frame_idx and status: the
    dict gains "score" [M], "keep" [M] uint8, "order" [M] int32, "n_keep" [1] int32 and "suppressed_by" [M] (and "oks" with
    want_matrix).  Shapes stay [M], nothing is compacted or read back, so a capture stays valid; at most 4096 boxes a call with nms."""
    nms_args = None
    if nms is not None and nms is not False:
        nms_args = {} if nms is True else dict(nms)
        bad = sorted(set(nms_args) - {"sigmas", "oks_thr", "vis_thr", "want_matrix"})
        if bad:
            raise ValueError(f"nms: {bad} are not oks_nms arguments predict() passes on (sigmas, oks_thr, vis_thr, want_matrix)")
    elif box_scores is not None:
        raise ValueError("box_scores are used by the rescoring of nms: give nms=True or a dict")
    Ho, Wo = data_gpu._crop_size(256 if input_size is None else input_size)
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    bd, fd, _ = data_gpu.box_inputs(frames_u8, boxes, frame_idx)
    data_gpu._check_frame_size(frames_u8)
    dev = frames_u8.device
    K = model.num_keypoints
    perm = kd._perm_device(flip_pairs, K, dev) if flip_pairs is not None else None      # (a bad table fails here, before any launch)
    fused = perm is not None and isinstance(decode, str) and decode == "argmax"
    md, sd = data_gpu._norm_consts(dev, mean, std)
    M = bd.shape[0]
    if nms_args is not None:
        if M > kd.NMS_MAX_POSES:
            raise ValueError(f"nms takes at most {kd.NMS_MAX_POSES} boxes a call, got {M}")
        if box_scores is not None and not torch.is_tensor(box_scores):
            box_scores = torch.from_numpy(np.ascontiguousarray(box_scores, dtype=np.float32)).to(dev, non_blocking=True)
    keypoints = torch.empty(M, K, 2, dtype=torch.float32, device=dev)
    confidence = torch.empty(M, K, dtype=torch.float32, device=dev)
    status = torch.empty(M, dtype=torch.uint8, device=dev)
    heatmaps = None
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for i0 in range(0, M, batch):
                n = min(batch, M - i0)
                b, fi = bd[i0:i0 + n], fd[i0:i0 + n]
                if n < batch:
                    b = torch.cat([b, b[:1].expand(batch - n, 5)]).contiguous()
                    fi = torch.cat([fi, fi[:1].expand(batch - n)]).contiguous()
                x, _, st = data_gpu.box_crop_launch(frames_u8, b, fi, Ho, Wo, md, sd, perm is not None, True, False)
                if perm is not None:
                    y2 = model(x)
                    y, preds, maxv = kd._flip_merge(y2[:batch], y2[batch:], perm, shift_heatmap, fused, out=y2[:batch])
                    if fused:
                        maxv = maxv.reshape(batch, K)
                    else:
                        preds, maxv = kd._decode_pred_max(y, decode)
                else:
                    y = model(x).float().contiguous()
                    preds, maxv = kd._decode_pred_max(y, decode)
                Hh, Wh = y.shape[2:]
                keypoints[i0:i0 + n] = kd._coords_to_image(preds, b, Ho, Wo, Wo / Wh, Ho / Hh)[:n]
                confidence[i0:i0 + n] = maxv[:n]
                status[i0:i0 + n] = st[:n]
                if return_heatmaps:
                    if heatmaps is None:
                        heatmaps = torch.empty(M, K, Hh, Wh, dtype=torch.float32, device=dev)
                    heatmaps[i0:i0 + n] = y[:n]
    finally:
        if was_training:
            model.train()
    out = {"keypoints": keypoints, "confidence": confidence, "status": status}
    if return_heatmaps:
        out["heatmaps"] = heatmaps
    if nms_args is not None:
        res = kd.oks_nms(keypoints, confidence, bd, frame_idx=fd, status=status, box_scores=box_scores, **nms_args)
        out.update({k: res[k] for k in ("score", "keep", "order", "n_keep", "suppressed_by", "oks") if k in res})
    if not torch.cuda.is_current_stream_capturing():
        sat = mt.split_saturations(reset=True)          # (as validate(): the evaluation forward runs the f16x2 mode under 'auto')
        if sat:
            import warnings
            warnings.warn(f"predict(): {sat} f16x2 stores saturated at |x| = 65504 (or were NaN) since the last check - activations outside "
                          "fp16's range; run the model with precision='fp32' (exact, slower) to rule the format out")
    return out


def evaluate_ap(batches, model, meter=None, nms=True, **predict_kwargs):
    """Key-point AP under OKS of predict()'s poses over a labelled set: per batch `predict(..., nms=nms)` and
    lib.keypoint_detection.APMeter.update_predict, then the meter's report - AP / AP50 / AP75 / APM / APL / AR and the tables.  Each batch
    is a dict: "frames" [F,Hs,Ws,3] uint8 CUDA, "boxes" [M,5], "frame_idx" [M] (the frame of every box, within the batch's frames),
    "box_scores" [M] (or None), and the labelled poses of those frames "gt_keypoints" [G,K,2] in frame pixels, "gt_visible" [G,K],
    "gt_area" [G], "gt_frame" [G], optionally "gt_ignore" [G].  meter: an APMeter to add to (None: one with the defaults for the model's key
    points); nms: True or a dict of oks_nms's arguments, as predict() takes it; predict_kwargs go to predict().  Nothing is read back before
    the report."""
    if nms is None or nms is False:
        raise ValueError("evaluate_ap() scores predict()'s rescored, thinned poses: nms must be True or a dict of oks_nms's arguments")
    dev = next(model.parameters()).device
    if meter is None:
        meter = kd.APMeter(model.num_keypoints, sigmas=nms.get("sigmas") if isinstance(nms, dict) else None, device=dev)
    for batch in batches:
        fi = batch["frame_idx"]
        if not torch.is_tensor(fi):
            fi = torch.from_numpy(np.ascontiguousarray(fi, dtype=np.int32)).to(dev, non_blocking=True)
        res = predict(batch["frames"], batch["boxes"], model, frame_idx=fi, box_scores=batch.get("box_scores"), nms=nms, **predict_kwargs)
        meter.update_predict(res, fi, batch["gt_keypoints"], batch["gt_visible"], batch["gt_area"], batch["gt_frame"],
                             num_frames=batch["frames"].shape[0], gt_ignore=batch.get("gt_ignore"))
    return meter.compute()


class GraphedTrainStep:
    """The mean-teacher step captured into hipGraphs: ~1300 kernel launches per step are replayed by ONE graph launch on one
    rank (forwards, losses, backward, Adam + EMA + packs), which removes the host launch gaps.
    Data parallel: four graphs - forwards | losses + backward part 1 | backward part 2 | Adam + EMA - with the confidence
    all-gather after the first, the all-reduce of the finished gradient suffix launched after the second (it runs on the
    communicator's stream under the third) and the small prefix all-reduce after the third.
    Inputs are copied into static device tensors before each replay; the re-warp matrices are computed INSIDE the captured step
    (udapose_recon_thetas, double precision) from the batch's raw aug_param values, which the host packs into a pinned ring and
    uploads with one asynchronous copy per step.
    Style transfer (train_human.py:345-358): each direction is its own small graph (content, style, alpha as a device scalar ->
    the step's effective input); the host draws the step's decisions in the reference's order and replays the direction(s) it
    drew, or copies the original images, before the main graph.  Occlusion (train_human.py:374-412): the decisions are taken
    on the device from four uniform draws per sample (trainer.device_occlusion), inside the main graph.
    Teacher views (train_human.py:361-372, `--k`): x_t_tea is one tensor, or a list / tuple of k <= 8 tensors [N,3,H,W] with aug_param_tea a
    list of k collated tuples - here and in step() / step_async() / prefetch().  k is fixed at construction (a later call with another count:
    ValueError).  Every view has its own static image buffer, effective-input buffer and re-warp matrices; the aug buffer is [1+k,N,6], still
    one copy per step; the k teacher forwards, their re-warps and the one mean_views / merge_views launch stay on the teacher's stream, in
    order, as in the eager step (the teacher's BatchNorm statistics advance k times).  trainer.view_merge needs k >= 2; a captured merge
    follows trainer.view_radius (step() calls sync_view_radius()); view_merge, view_min and k are frozen.  Style: one pair of draws per step;
    every view is summarised only when t2s was drawn (the first otherwise), t2s transfers every view into its own buffer.
    Scheduled values (trainer.scheduled): lambda_c / lambda_ent / lambda_coral, teacher_alpha and mask_ratio named there are
    read from device memory by the captured launches; step() calls trainer.sync_schedule() before the replay, and changing them is no
    longer refused.  Names not listed stay frozen, and so does the list itself.
    Mirrored views: built with trainer.flip_pairs set, the step keeps a static uint8 [1+k,N] buffer of flip flags, staged per step
    like the aug_param values, and captures the mirrored form of every warp: a replay follows the flags of its batch (4-entry aug_params stage
    zeros, and a sample whose flag is 0 gets the bits of the plain launch).  Built without, it captures the plain launches and refuses a batch
    with a flagged sample (ValueError).  flip_pairs is frozen."""

    mirrored = False            # built with trainer.flip_pairs set: the mirrored launch forms are captured and the flags staged per step
    k, _sfx = 1, [""]           # teacher views per step, and the suffix of view i's static keys ("" for view 0): set by the constructor

    def __init__(self, trainer, x_s, label_s, weight_s, x_t_stu, x_t_tea, aug_param_stu, aug_param_tea, warmup=2, split=None, metrics=True,
                 capture_comm=None):
        # metrics: the captured step also decodes y_s and computes PCK@0.05 against label_s on the device (the reference's per-iteration
        # `accuracy(y_s, label_s)`, train_human.py:443) and gathers the losses + PCK into ONE small device vector: step_async() reads
        # it back one step late through a pinned double buffer, so a loop that logs every iteration never drains the device
        self.t = trainer
        self.metrics = bool(metrics)
        self._mvec, self._mpin, self._mev, self._mi, self._mk, self._macc, self._mextra = None, None, [None, None], 0, 0, None, []
        # other threads (the RCCL watchdog of torch.distributed) may touch the runtime while this thread captures
        self._mode = "thread_local" if _dist_on() else "global"
        x_t_tea, aug_param_tea = self._views(x_t_tea, aug_param_tea, fix_k=True)
        self._refuse_uncapturable(x_t_stu)
        self._allocate_static(x_s, label_s, weight_s, x_t_stu, x_t_tea, aug_param_stu, aug_param_tea)
        self._warm_up(warmup)
        self._settle_watchdog(capture_comm)
        self._capture_style()
        self._decide_form(split, capture_comm)
        if self.split or not self._capture_whole():
            self._capture_split()
        self._capture_update()
        self._after_capture()

    @staticmethod
    def _is_collated(ap):
        """One collated aug_param, (angle, (tx, ty), (shear_x, shear_y), scale) - as against a list of them, one per view."""
        try:
            return len(ap) in (4, 5) and len(ap[1]) == 2 and len(ap[2]) == 2       # (5: with the flip flags of mirrored views)
        except TypeError:
            return False

    def _views(self, x_t_tea, aug_param_tea, fix_k=False):
        """The two call forms of the teacher's side -> (list of k images | None, list of k collated aug_params | None).  fix_k: the
        constructor's call, which sets self.k; afterwards another count is a ValueError naming both."""
        single = x_t_tea is not None and not isinstance(x_t_tea, (list, tuple))
        if single:
            x_t_tea = [x_t_tea]
        if aug_param_tea is not None:
            if self._is_collated(aug_param_tea):
                aug_param_tea = [aug_param_tea]
            elif single and not (isinstance(aug_param_tea, (list, tuple)) and len(aug_param_tea) > 0
                                 and all(self._is_collated(ap) for ap in aug_param_tea)):
                # (with one image tensor anything that is not a list of collated tuples is taken as the tuple itself, as before:
                # pack_aug_param names what is wrong with it; a list of them is counted below)
                aug_param_tea = [aug_param_tea]
        for name, v in (("x_t_tea", x_t_tea), ("aug_param_tea", aug_param_tea)):
            if v is None:
                continue
            if len(v) > 8:
                raise NotImplementedError("at most 8 teacher views per step (the reference's --k defaults to 1)")
            if fix_k and name == "x_t_tea":
                if len(v) < 1:
                    raise ValueError("GraphedTrainStep: no teacher view given")
                self.k = len(v)
            if len(v) != self.k:
                raise ValueError(f"GraphedTrainStep was built with k = {self.k} teacher view(s) per step and is called with {len(v)} in {name}: "
                                 "k is fixed at construction - build a new GraphedTrainStep for another count")
        return (list(x_t_tea) if x_t_tea is not None else None), (list(aug_param_tea) if aug_param_tea is not None else None)

    def _refuse_uncapturable(self, x_t_stu):
        t = self.t
        self._style = _StyleAdapter(t.style_net, captured=True) if t.style_net is not None else None     # (TypeError: a net with the plain call only)
        if t.view_merge is not None and self.k < 2:
            raise ValueError(f"GraphedTrainStep was given a single teacher view per step, and trainer.view_merge = {t.view_merge!r} merges "
                             "k >= 2 of them: pass a list of k >= 2 target views (and their aug_params), or set trainer.view_merge = None "
                             "before building the captured step")
        t._check_view_merge(self.k)         # (a mode warp.merge_views does not know)
        t._scheduled_names()                # (ValueError: a name that cannot be scheduled)
        self.styled, self.occl = self._style is not None, t.occlude_rate > -1
        if self.occl and not t.device_occlusion:
            raise RuntimeError("GraphedTrainStep with occlusion needs trainer.device_occlusion = True (the reference's host draws read "
                               "the confidences back every step, which a captured step cannot do)")
        if t.warp_mode == "bilinear":
            hm = [int(round(v / t.ratio)) for v in x_t_stu.shape[-2:]]
            if not warp.bilinear_fits_lds(*hm):
                raise RuntimeError(f"GraphedTrainStep with warp_mode='bilinear': {hm[0]}x{hm[1]} heat-map planes exceed the re-warp's "
                                   f"{warp.BILINEAR_LDS_BYTES // 1024} KB LDS budget; the stage-by-stage form allocates scratch memory, which a "
                                   "captured step must not do - use the eager train_step for heat-maps this large")

    def _allocate_static(self, x_s, label_s, weight_s, x_t_stu, x_t_tea, aug_param_stu, aug_param_tea):
        self._stage, self._have_staged = None, False
        dev, n = x_s.device, x_s.shape[0]
        self.n = n
        # The re-warp matrices are computed INSIDE the captured step (udapose_recon_thetas, double precision) from the batch's raw
        # aug_param values: per step the host packs (1 + k) x N x 6 doubles into a pinned buffer and issues one asynchronous copy.
        # View i of the teacher has the static keys x_t_tea / x_t_tea_in / theta_tea with the suffix "" (view 0) or str(i).
        k = self.k
        self._sfx = [""] + [str(i) for i in range(1, k)]
        self._in_keys = _INPUTS[:4] + tuple("x_t_tea" + s for s in self._sfx)
        st = self.static = {key: v.clone() for key, v in zip(self._in_keys, (x_s, label_s, weight_s, x_t_stu) + tuple(x_t_tea))}
        st.update(aug=torch.empty(1 + k, n, 6, dtype=torch.float64, device=dev), theta_stu=torch.empty(n, 3, 6, dtype=torch.float32, device=dev))
        for s in self._sfx:
            st["theta_tea" + s] = torch.empty(n, 3, 6, dtype=torch.float32, device=dev)
        self._aug_pin = [torch.empty(1 + k, n, 6, dtype=torch.float64).pin_memory() for _ in range(4)]
        self._aug_ev, self._aug_i, self._aug_last = [None] * 4, 0, None
        # mirrored views: the flip flags of the student's view and of the k teacher views, staged through a pinned ring beside `aug`
        self.mirrored = self.t.flip_pairs is not None
        if self.mirrored:
            st["mirror"] = torch.zeros(1 + k, n, dtype=torch.uint8, device=dev)
            self._mir_pin = [torch.zeros(1 + k, n, dtype=torch.uint8).pin_memory() for _ in range(4)]
            self._mir_last = None
            warp.mirror_perm(self.t.flip_pairs, label_s.shape[1], dev)      # (uploaded here, outside any capture; ValueError: a bad table)
        self._stage_aug(aug_param_stu, aug_param_tea)
        # the main graph reads the step's EFFECTIVE inputs: the originals, or what the style graphs wrote
        st["x_s_in"] = st["x_s"].clone() if self.styled else st["x_s"]
        for s in self._sfx:
            st["x_t_tea_in" + s] = st["x_t_tea" + s].clone() if self.styled else st["x_t_tea" + s]
        if self.styled:
            st["alpha_s2t"] = torch.ones(1, dtype=torch.float32, device=dev)
            st["alpha_t2s"] = torch.ones(1, dtype=torch.float32, device=dev)
        if self.occl:
            st["theta_back"] = torch.empty(n, 1, 6, dtype=torch.float32, device=dev)
            st["u"] = torch.zeros(n, 4, dtype=torch.float32, device=dev)
        self.t._occl = ("device", st["theta_back"], st["u"]) if self.occl else None

    def _step_args(self):
        """What the trainer's _forward_backward / _forward_part are called with, in the warm-up steps and in every capture."""
        st = self.static
        args = (st["x_s_in"], st["label_s"], st["weight_s"], st["x_t_stu"], [st["x_t_tea_in" + s] for s in self._sfx], st["theta_stu"],
                [st["theta_tea" + s] for s in self._sfx])
        if self.mirrored:       # the static flip flags of the student's view and of the k teacher views
            args += (st["mirror"][0], [st["mirror"][1 + i] for i in range(self.k)])
        return args

    def _warm_up(self, warmup):
        t, dev = self.t, self.static["x_s"].device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        self.g_style = {}
        self._cap = {"stream": torch.cuda.Stream(device=dev, priority=t.stream_priority)} if t.stream_priority else {}
        with torch.cuda.stream(side):
            for which in self._style_graphs():      # (the style net's plans and packs; no model state involved)
                self._style_pass(which)
            for _ in range(warmup):     # REAL steps (same host draws as step()): fill the plan / table caches, allocator steady state
                self._thetas()
                self._draw_and_style()
                t._forward_backward(*self._step_args())
                t._sync_grads()
                t._update()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def _settle_watchdog(self, capture_comm):
        # RCCL's watchdog thread polls the end events of the EAGER collectives issued so far (the warm-up steps'); on this HIP an
        # event query fails with hipErrorCapturedEvent once the communicator's stream has joined a capture, even for an event that
        # was recorded before it - and the watchdog then takes the process down.  Everything is complete here (synchronize above):
        # give the watchdog (100 ms poll) time to retire those works before any collective is captured.  torch exposes no call that
        # waits for the watchdog's list to drain, so this IS a timed wait (ten polls) - which is why capturing the
        # collectives is opt-in (capture_comm below) and why the capture's failure path falls back to eager collectives.
        if _dist_on() and dist.get_backend() == "nccl" and (
                capture_comm or (capture_comm is None and os.environ.get("UDAPOSE_CAPTURE_COMM", "0") == "1")):
            import time
            dist.barrier()
            torch.cuda.synchronize()
            time.sleep(1.0)

    @contextlib.contextmanager
    def _capturing(self, g, pool=None, whole=False, origin=True):
        """`with` this: the body is captured into the graph g.  whole: g holds the losses of a one-graph step, whose metrics are computed on a
        side stream under the backward (_metrics_side).  origin=False: the style graphs, captured on torch's own capture stream."""
        if whole and self.one_graph and self.metrics:
            self.t._metrics_cb = self._metrics_side
        try:
            with torch.cuda.graph(g, capture_error_mode=self._mode, pool=pool, **(self._cap if origin else {})):
                yield
        finally:
            self.t._metrics_cb = None

    def _style_graphs(self):
        """The style graphs of this step, in the order they are first run: "enc_rest" (the summaries of views 1 .. k-1, needed by t2s alone)
        exists only with k >= 2."""
        if not self.styled:
            return ()
        return ("enc",) + (("enc_rest",) if self.k > 1 else ()) + ("s2t", "t2s")

    def _capture_style(self):
        for which in self._style_graphs():
            g = torch.cuda.CUDAGraph()
            with self._capturing(g, pool=self.g_style["enc"].pool() if self.g_style else None, origin=False):
                self._style_pass(which)
            self.g_style[which] = g

    def _decide_form(self, split, capture_comm):
        t = self.t
        # capture_comm (round 5): the step's collectives - confidence all-gather, gradient all-reduce buckets - are captured INTO the step's
        # graph (RCCL launches are stream-ordered kernels: capturable), so the data-parallel step is ONE graph launch like the one-rank step
        # instead of four graphs with eager collectives between them.  OPT-IN (round 6, ADVICE r5: the argument, or UDAPOSE_CAPTURE_COMM=1):
        # it rests on a timed wait for RCCL's watchdog (above), replayed collectives are invisible to torch.distributed's timeout, and no
        # multi-GPU node has run it yet; bench.py --gpus N asks for it explicitly (with its own hang guard) and lets the ranks fall back
        # together.  If the capture raises (a collective backend that cannot be captured), the four-graph form is built instead.
        if capture_comm is None:
            capture_comm = (_dist_on() and dist.get_backend() == "nccl" and split is None
                            and os.environ.get("UDAPOSE_CAPTURE_COMM", "0") == "1")
        self.capture_comm = bool(capture_comm) and _dist_on()
        if self.capture_comm and t.sync.comm_dtype == "bf16" and t._overlap():
            # the bf16 exchange of the suffix runs on a side stream that hands over to the communicator's stream and waits for it again:
            # a fork that waits back on a non-origin stream brings hipStreamEndCapture down on this ROCm (tools/capture_fork_patterns.py)
            self.capture_comm = False
        t.capture_comm = self.capture_comm
        self.split = (_dist_on() and not self.capture_comm) if split is None else bool(split)
        # hyper-parameters that are kernel ARGUMENTS of the captured launches stay what they were at capture: step() checks
        # them.  (lr / grad_scale are read from device memory and follow the optimizer's param_groups, see optim.py.)
        self._frozen = self._frozen_hyper()
        if t.mask_mode == "threshold":
            t.sync_mask_threshold(self.static["x_s"].device)    # (the captured mask launch reads this scalar: it exists, and is current, before the capture)
        if t.adv_eps is not None:
            t.sync_adv(self.static["x_s"].device)               # (likewise the perturbation's eps / step)
        if t.view_merge is not None:
            t.sync_view_radius(self.static["x_s"].device)       # (likewise the merge's radius)
        if t.scheduled:
            t.sync_schedule(self.static["x_s"].device)          # (likewise the words of the scheduled values)
        t.student._capture_token = t.teacher._capture_token = object()      # weight packs: captured once per network, unconditionally (pose_resnet._pack)
        self.g_fb, self.g_lb, self.g_lb2, self.g_up = torch.cuda.CUDAGraph(), None, None, None
        # overlap: the backward is cut after layer3 (two graph segments) and the finished gradient suffix is all-reduced on
        # the communicator's stream while the second segment replays
        self.overlap = t._overlap()
        # one rank, nothing eager between backward and the optimizer: the update is captured into the same graph (one launch per step)
        self.one_graph = (not self.split) and (self.capture_comm or not _dist_on()) and t.single_graph
        self.capture_fallback = None        # why the captured-collectives form was given up (None: it was not, or was never asked for)

    def _capture_whole(self):
        """The unsplit step in self.g_fb: forwards, losses, backward; with capture_comm its collectives too; with one_graph also Adam + EMA + packs and
        the metrics.  False: some rank could not capture the collectives - all is cleaned up here and every rank builds the split form instead."""
        t, e = self.t, None
        try:
            if self.capture_comm and os.environ.get("UDAPOSE_TEST_FAIL_CAPTURE", "0") == "1":     # test hook (tests/test_gpu_hotpath.py): the collective fallback
                raise RuntimeError("injected capture failure (UDAPOSE_TEST_FAIL_CAPTURE=1)")
            with self._capturing(self.g_fb, whole=True):
                self._thetas()
                self.out = t._forward_backward(*self._step_args())
                if self.capture_comm or self.one_graph:
                    # captured collectives: backward part 2 under the suffix's all-reduce, then the prefix's.  One rank: the collectives are
                    # no-ops, what is left is _backward_lower() where part 2 is pending (overlap forced: both parts in the one graph)
                    t._sync_grads()
                elif t.student._pending_lower:      # (part 2 of a forced overlap; what follows it stays eager: _capture_update)
                    t._backward_lower()
                if self.one_graph:
                    t._update()
                    self._capture_metrics()
        except Exception as e_:      # (the backend refused the capture: fall back to eager collectives between four graphs)
            if not self.capture_comm:
                raise
            e = e_
        if not self.capture_comm:
            return True
        # The fallback is a COLLECTIVE decision: a rank that kept its captured graph while another replays eager collectives would pair
        # them wrongly and hang.  Every rank reports, the minimum decides (one eager all-reduce, outside any capture).
        ok_all = e is None
        if dist.is_available() and dist.is_initialized() and not torch.cuda.is_current_stream_capturing():
            flag = torch.tensor([1.0 if ok_all else 0.0], device=self.static["x_s"].device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            ok_all = bool(flag.item() >= 1.0)
        if ok_all:
            return True
        import warnings
        why = f"{type(e).__name__}: {e}" if e is not None else "another rank could not capture the collectives"
        self.capture_fallback = why
        warnings.warn(f"GraphedTrainStep: capturing the collectives into the step's graph failed ({why}); "
                      "every rank uses the four-graph form with eager collectives")
        t.capture_comm = self.capture_comm = False
        self._macc = None
        # whatever the aborted capture left half-done: the four-graph form starts from a clean executor and a clean GradSync
        t.student._drop_pending_step()
        t.sync.reset()
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GraphedTrainStep: the failed capture of the collectives left the stream capturing; cannot fall back")
        torch.cuda.synchronize()
        self.g_fb = torch.cuda.CUDAGraph()
        self.split, self.one_graph = True, False
        return False

    def _capture_split(self):
        """g_fb | eager all-gather | g_lb | [eager start of the suffix's all-reduce | g_lb2]; the other collectives and g_up: _capture_update."""
        self.g_lb = torch.cuda.CUDAGraph()
        with self._capturing(self.g_fb):
            self._thetas()
            self.fwd_state = self.t._forward_part(*self._step_args())
        g0 = gather_activates(self.fwd_state["activates"])
        self.gathered = g0.clone() if g0 is not None else self.fwd_state["activates"].reshape(-1).clone()
        with self._capturing(self.g_lb, pool=self.g_fb.pool()):
            self.out = self.t._loss_backward_part(self.fwd_state, self.gathered)
        if self.overlap:
            self.t.sync.start_upper()
            self.g_lb2 = torch.cuda.CUDAGraph()
            with self._capturing(self.g_lb2, pool=self.g_fb.pool()):
                self.t._backward_lower()

    def _capture_update(self):
        if self.one_graph:
            return
        self.g_up = torch.cuda.CUDAGraph()
        if not self.capture_comm:           # (captured collectives are inside g_fb)
            (self.t.sync.finish if self.g_lb2 is not None else self.t.sync)()
        with self._capturing(self.g_up, pool=self.g_fb.pool()):
            self.t._update()
            self._capture_metrics()

    def _after_capture(self):
        t = self.t
        t.student._capture_token = t.teacher._capture_token = None
        self._opt_key = self._optimizer_key()
        self._fused_tail = bool(t.fused_last)
        self._maintained = [(t.student, t.student._last_hd, True), (t.teacher, t.teacher._last_hd, False)]
        self._weights_moved()
        torch.cuda.synchronize()

    def _weights_moved(self):
        # the captured Adam / EMA kernels changed both networks' parameters behind torch's back: every executor plan (other batch sizes,
        # validate(), fp32 mode) must re-pack its bf16 weights before its next forward ...
        for m, hd, bwd in self._maintained:
            m.weights_changed()
            if self._fused_tail:          # ... but the step's own plans, whose packs the captured update has just rewritten
                m.packs_refreshed(hd, bwd)

    def _drop_graphs(self):
        self.g_fb = self.g_lb = self.g_lb2 = self.g_up = None

    def release(self):
        """Destroy the captured graphs.  With capture_comm the graphs hold RCCL launches, and RCCL's communicator teardown waits for every
        such graph to be gone: call this (or drop every reference to the object) BEFORE torch.distributed.destroy_process_group(), which
        otherwise never returns (measured on RCCL 2.26 / ROCm 7.0)."""
        self._drop_graphs()
        self.g_style = {}
        import gc
        gc.collect()
        torch.cuda.synchronize()

    def __del__(self):
        # (graphs that captured RCCL launches must be gone before destroy_process_group(): dropping the last reference does what release() does)
        try:
            if getattr(self, "capture_comm", False):
                self._drop_graphs()
        except Exception:
            pass

    def _capture_metrics(self):
        """(inside the capture of the step's last graph) losses + device PCK of the source batch -> self._mvec = [loss_all, loss_s, loss_c,
        avg_acc, cnt, acc[0..K-1]]: decode and PCK are the udapose_heatmap_argmax / udapose_pck launches of lib.keypoint_detection."""
        if not self.metrics:
            return
        if self._macc is not None:          # computed on the side stream while the backward ran: join it
            torch.cuda.current_stream().wait_stream(self._macc[2])
            acc, avg_cnt = self._macc[0], self._macc[1]
            for t in (acc, avg_cnt):
                t.record_stream(torch.cuda.current_stream())
        else:
            acc, avg_cnt, _ = kd.accuracy_device(self.out["y_s"], self.static["label_s"])
        parts = [self.out["loss_all"].reshape(1), self.out["loss_s"].reshape(1), self.out["loss_c"].reshape(1), avg_cnt.reshape(2), acc.reshape(-1)]
        opt = self.t.stu_optimizer
        if getattr(opt, "max_grad_norm", None) is not None:       # (the captured update has just written it: the norm before clipping)
            self.out["grad_norm"] = opt.grad_norm()
        self._mextra = [k for k in ("loss_ent", "loss_coral", "grad_norm") if k in self.out]      # (appended in this order: the layout without them is unchanged)
        parts += [self.out[k].reshape(1) for k in self._mextra]
        self._mk = int(acc.numel())
        self._mvec = torch.cat([p.float() for p in parts])
        self.out["acc_s"], self.out["acc_avg_cnt"] = acc, avg_cnt

    def _metrics_side(self, st):
        """(inside the one-graph capture, called by the trainer before the losses) the metric's decode + PCK launches on the teacher's
        stream, which is idle from here on: they run under the backward instead of behind the optimizer tail (pck_k alone is a 24 us
        single-work-group kernel)."""
        t = self.t
        side = t._side[0] if (t._side is not None and t.concurrent) else None
        if side is None:
            return
        main = torch.cuda.current_stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):
            acc, avg_cnt, _ = kd.accuracy_device(st["y_s"], self.static["label_s"])
        st["y_s"].record_stream(side)
        self._macc = (acc, avg_cnt, side)

    def _metrics_dict(self, v):
        v = v.tolist()
        d = {"loss_all": v[0], "loss_s": v[1], "loss_c": v[2], "acc_s": v[3], "cnt_s": int(v[4]), "acc_per_keypoint": v[5:5 + self._mk]}
        for i, k in enumerate(self._mextra):
            d[k] = v[5 + self._mk + i]
        return d

    def step_async(self, *args, **kw):
        """step() with the metric read-back DEFERRED by one step: replays this step, queues the copy of its metric vector into a pinned
        slot behind it, and only then waits for the PREVIOUS step's slot - the device always has the next replay queued while the host
        reads, so the reference's per-iteration logging (train_human.py:440-452) costs no device idle time (a synchronous read exposes
        the ~0.75 ms launch latency of a 1270-node graph every step).  Returns the previous step's metrics as Python numbers (None on
        the first call); flush_metrics() returns the last step's."""
        if self._mvec is None:
            raise RuntimeError("GraphedTrainStep(metrics=False) has no metric vector to read back")
        if self._mpin is None:
            self._mpin = [torch.empty(self._mvec.numel(), dtype=torch.float32).pin_memory() for _ in range(2)]
        self.step(*args, **kw)
        i = self._mi
        self._mpin[i].copy_(self._mvec, non_blocking=True)
        self._mev[i] = torch.cuda.Event()
        self._mev[i].record()
        self._mi = 1 - i
        return self._read_slot(1 - i)

    def _read_slot(self, i):
        """Wait for metric slot i, clear it and decode it (None: nothing is queued in it)."""
        ev, self._mev[i] = self._mev[i], None
        if ev is None:
            return None
        ev.synchronize()
        return self._metrics_dict(self._mpin[i])

    def flush_metrics(self):
        """Metrics of the most recent step_async() (waits for it)."""
        return self._read_slot(1 - self._mi)

    profile_segments = False        # bench.py --dp-segments: HIP events between the parts of a step (device time per part, after a synchronize)

    def _seg_mark(self, name):
        if not self.profile_segments:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.__dict__.setdefault("_seg_events", []).append((name, e))

    def segment_ms(self):
        """Mean device time of each part of the step since the last call: {part: ms} (the parts of one step are consecutive events)."""
        ev = self.__dict__.pop("_seg_events", [])
        torch.cuda.synchronize()
        tot, cnt = {}, {}
        for (n0, e0), (n1, e1) in zip(ev, ev[1:]):
            if n1 == "start":
                continue
            tot[n1] = tot.get(n1, 0.0) + e0.elapsed_time(e1)
            cnt[n1] = cnt.get(n1, 0) + 1
        return {k: round(tot[k] / cnt[k], 3) for k in tot}

    def _stage_aug(self, aug_param_stu=None, aug_param_tea=None):
        """The batch's raw aug_param values -> the static [1+k,N,6] float64 device buffer the captured udapose_recon_thetas launches
        read (a ring of pinned host buffers and one asynchronous copy: nothing here waits for the device).  aug_param_tea: a list of k."""
        if aug_param_stu is None and aug_param_tea is None:
            return
        flags = [warp.aug_mirror(ap, self.n) if ap is not None else None for ap in [aug_param_stu] + list(aug_param_tea or [None] * self.k)]
        if not self.mirrored and any(f is not None and bool(f.any()) for f in flags):
            raise ValueError("GraphedTrainStep was built without trainer.flip_pairs and captured the un-mirrored warps: it cannot take a batch "
                             "with flipped samples - set trainer.flip_pairs and build a new GraphedTrainStep")
        i = self._aug_i = (self._aug_i + 1) % len(self._aug_pin)
        if self._aug_ev[i] is not None:
            self._aug_ev[i].synchronize()             # (the copy issued from this slot four steps ago: long done)
        pin = self._aug_pin[i]
        if self._aug_last is not None:
            pin.copy_(self._aug_last)                 # a side that is not given keeps its previous values
        if aug_param_stu is not None:
            warp.pack_aug_param(aug_param_stu, self.n, out=pin[0])
        for v, ap in enumerate(aug_param_tea or ()):      # (view v; `i` stays the ring slot the event below is kept in)
            warp.pack_aug_param(ap, self.n, out=pin[1 + v])
        self.static["aug"].copy_(pin, non_blocking=True)
        if self.mirrored:
            mpin = self._mir_pin[i]
            if self._mir_last is not None:
                mpin.copy_(self._mir_last)
            for v, (ap, f) in enumerate(zip([aug_param_stu] + list(aug_param_tea or [None] * self.k), flags)):
                if ap is not None:                    # (a 4-entry aug_param: an un-mirrored view, zeros)
                    mpin[v] = f if f is not None else 0
            self.static["mirror"].copy_(mpin, non_blocking=True)
            self._mir_last = mpin
        ev = torch.cuda.Event()
        ev.record()
        self._aug_ev[i], self._aug_last = ev, pin

    def _thetas(self):
        """Launch the matrix kernels (captured: at the head of the step's first graph) from the static aug buffer.  (Round 4 tried them on a
        stream of their own, beside the forwards: no measurable gain, and the earlier start of the three branches changed the arrival order
        of the stem's fp32 atomics often enough to break the bit-for-bit twins of tests/test_gpu_steps.py; reverted.)"""
        st, r = self.static, self.t.ratio
        warp.thetas_from_packed(st["aug"][0], r, want_fwd=True, want_back=self.occl, fwd=st["theta_stu"], back=st.get("theta_back"))
        for i, s in enumerate(self._sfx):
            warp.thetas_from_packed(st["aug"][1 + i], r, fwd=st["theta_tea" + s])

    def _style_pass(self, which):
        """"enc": the summaries (_StyleAdapter: relu4_1 features, or low-frequency spectra) of both ORIGINAL batches into static buffers, once per
        step whichever directions are drawn ("enc_rest": of the teacher's views 1 .. k-1, when t2s was drawn - _style_part's rule);
        "s2t" / "t2s": one direction's transfer from those summaries into the main graph's input buffer(s), t2s for every view."""
        if which in self.g_style:       # (captured by now: replay it)
            return self.g_style[which].replay()
        st, style, (k_s, k_t) = self.static, self._style, self._style.keys
        with torch.no_grad():
            if which in ("enc", "enc_rest"):
                todo = (("x_s", k_s), ("x_t_tea", k_t)) if which == "enc" else tuple(("x_t_tea" + s, k_t + s) for s in self._sfx[1:])
                for img, key in todo:
                    if key in st:
                        style.summarize(st[img], out=st[key])
                    else:       # (the first, uncaptured pass: a buffer of its own, not the net's arena)
                        st[key] = style.summarize(st[img]).clone()
            elif which == "s2t":
                style.transfer(st["x_s"], st[k_s], st[k_t], st["alpha_s2t"], self.t.recover, out=st["x_s_in"])
            else:
                for s in self._sfx:
                    style.transfer(st["x_t_tea" + s], st[k_t + s], st[k_s], st["alpha_t2s"], self.t.recover, out=st["x_t_tea_in" + s])

    def _draw_and_style(self):
        """The step's host draws, in the eager step's (= the reference's) order, and what follows from them: each style direction drawn runs (its
        graph once captured) into the main graph's input buffer, the other keeps the original images; the occlusion's uniform numbers go to the device."""
        st = self.static
        if self.styled:
            decisions = self.t.draw_style_decisions()
            if any(a is not None for a in decisions):
                self._style_pass("enc")
                if decisions[1] is not None and self.k > 1:
                    self._style_pass("enc_rest")
            pairs = ((("x_s_in", "x_s"),), tuple(("x_t_tea_in" + s, "x_t_tea" + s) for s in self._sfx))
            for which, a, srcs in zip(("s2t", "t2s"), decisions, pairs):
                if a is not None:
                    st["alpha_" + which].fill_(float(a))
                    self._style_pass(which)
                else:
                    for dst, src in srcs:
                        st[dst].copy_(st[src], non_blocking=True)
        if self.occl:
            st["u"].copy_(self.t.draw_occlusion_uniforms(self.n), non_blocking=True)

    def _optimizer_key(self):
        """Storage the captured optimizer launches point at: the device state of every group and the first moment tensor; with clipping by
        global norm its device buffer and the per-block partial sums."""
        opt = self.t.stu_optimizer
        key = [ent[0].data_ptr() for _, ent in sorted(getattr(opt, "_dev", {}).items())]
        if getattr(opt, "max_grad_norm", None) is not None:
            key += [buf.data_ptr() for buf in (opt._clip[0] if opt._clip else None, opt._clip_part) if buf is not None]
        for g in opt.param_groups:
            for p in g["params"]:
                st = opt.state.get(p)
                if st:
                    key += [v.data_ptr() for v in st.values() if torch.is_tensor(v)]
                    break
        return key

    def _frozen_hyper(self):
        t, opt = self.t, self.t.stu_optimizer
        # a name in trainer.scheduled is read from device memory by the captured launches (sync_schedule) and may change freely; the list itself
        # decides which launches were captured and is frozen
        scheduled = t._scheduled_names()
        frozen = [("teacher_alpha", float(t.tea_optimizer.alpha)), ("lambda_c", float(t.lambda_c)), ("mask_ratio", float(t.mask_ratio))]
        frozen = [f for f in frozen if f[0] not in scheduled]
        frozen += [("sigma", float(t.sigma)), ("bn_momentum", float(t.student.bn_momentum)), ("occlude_rate", float(t.occlude_rate)),
                   ("occlude_thresh", float(t.occlude_thresh)), ("occlude_size", int(t.occlude_size)), ("warp_mode", str(t.warp_mode)),
                   ("scheduled", scheduled), ("flip_pairs", t.flip_pairs if t.flip_pairs is None or isinstance(t.flip_pairs, str)
                                              else tuple(tuple(int(v) for v in pr) for pr in t.flip_pairs))]
        for gi, g in enumerate(opt.param_groups):
            for k in ("betas", "eps", "weight_decay", "momentum", "nesterov"):
                if k in g:
                    frozen.append((f"group{gi}.{k}", g[k]))
        # clipping by global norm on / off changes the launches; its value lives on the device and may change freely (sync_hyper)
        frozen.append(("max_grad_norm enabled", getattr(opt, "max_grad_norm", None) is not None))
        # the mask's mode picks the launch; mask_threshold lives on the device and may change freely (sync_mask_threshold)
        frozen.append(("mask_mode", str(t.mask_mode)))
        # the adversarial view: on / off, the norm, the number of probes and whether a step is given pick the launches; adv_eps / adv_step
        # live on the device and may change freely (sync_adv)
        frozen += [("adv_eps enabled", t.adv_eps is not None), ("adv_norm", str(t.adv_norm)), ("adv_steps", int(t.adv_steps)),
                   ("adv_step given", t.adv_step is not None)]
        # the merge of k teacher views: on / off, the mode and view_min pick the launch and its arguments, k the static buffers; view_radius
        # lives on the device and may change freely (sync_view_radius)
        frozen += [("view_merge", t.view_merge), ("view_min", t.view_min), ("k", self.k)]
        for name, crit in (("criterion", t.criterion), ("con_criterion", t.con_criterion)):
            for k in ("topk", "largest"):
                if hasattr(crit, k):
                    frozen.append((f"{name}.{k}", getattr(crit, k)))
        return frozen

    def prefetch(self, x_s, label_s, weight_s, x_t_stu, x_t_tea):
        """Start copying the NEXT batch (pinned host tensors) into staging buffers on a copy stream; it overlaps with the
        replay of the current step.  The following step() call (with no tensors given) takes the staged batch with five
        device-to-device copies (92 MB, ~30 us) instead of waiting for PCIe on the compute stream.  x_t_tea: a tensor or a list of k."""
        x_t_tea, _ = self._views(x_t_tea, None)
        if self._stage is None:
            self._stage = {k: torch.empty_like(self.static[k]) for k in self._in_keys}
            self._copy_stream = torch.cuda.Stream(device=self.static["x_s"].device)
            self._staged, self._consumed = torch.cuda.Event(), None
        if self._consumed is not None:
            self._copy_stream.wait_event(self._consumed)     # the previous step's D2D reads of the staging buffers come first
        with torch.cuda.stream(self._copy_stream):
            for k, v in zip(self._in_keys, (x_s, label_s, weight_s, x_t_stu) + tuple(x_t_tea)):
                self._stage[k].copy_(v, non_blocking=True)
            self._staged.record(self._copy_stream)
        self._have_staged = True

    def step(self, x_s=None, label_s=None, weight_s=None, x_t_stu=None, x_t_tea=None, aug_param_stu=None, aug_param_tea=None):
        st = self.static
        x_t_tea, aug_param_tea = self._views(x_t_tea, aug_param_tea)
        if x_s is None and self._have_staged:
            torch.cuda.current_stream().wait_event(self._staged)
            for k in self._stage:
                st[k].copy_(self._stage[k], non_blocking=True)
            self._consumed = torch.cuda.Event()
            self._consumed.record()
            self._have_staged = False
        for k, v in zip(self._in_keys, (x_s, label_s, weight_s, x_t_stu) + tuple(x_t_tea or (None,) * self.k)):
            if v is not None and v.data_ptr() != st[k].data_ptr():
                st[k].copy_(v, non_blocking=True)
        self._stage_aug(aug_param_stu, aug_param_tea)
        frozen_now = self._frozen_hyper()
        if frozen_now != self._frozen:
            old, now = dict(self._frozen), dict(frozen_now)     # (by name: a change of trainer.scheduled moves names in and out of the list)
            changed = [n for n in now if n not in old or old[n] != now[n]] + [n for n in old if n not in now]
            raise RuntimeError(f"GraphedTrainStep: {changed} changed after capture; these are baked into the captured launches - "
                               "build a new GraphedTrainStep (lr and grad_scale may change freely)")
        if self._optimizer_key() != self._opt_key:
            raise RuntimeError("GraphedTrainStep: the optimizer's state tensors were replaced after capture (a new optimizer, or state moved to "
                               "another device): the captured launches still point at the old storage - build a new GraphedTrainStep "
                               "(FusedAdam / FusedSGD.load_state_dict restores IN PLACE and is fine)")
        if self._fused_tail:
            # the captured step relies on the packs its own previous update left: if anything else touched the weights since
            # (an eager optimizer, load_state_dict), re-pack eagerly first
            for m, hd, bwd in self._maintained:
                if hd.wpack_version is None or hd.wpack_version[0] != m.version_key():
                    hd.wpack_version = None
                    with torch.enable_grad() if bwd else torch.no_grad():
                        m.prepare(self.static["x_s"])
        self._draw_and_style()
        seg = self._seg_mark            # (profile_segments: an event after each part of the data-parallel step; a no-op otherwise)
        seg("start")
        if self.t.mask_mode == "threshold":
            self.t.sync_mask_threshold()         # a curriculum ramp of mask_threshold -> the device scalar the captured mask launch reads
        if self.t.adv_eps is not None:
            self.t.sync_adv()                    # adv_eps / adv_step -> the device scalars the captured perturb launches read
        if self.t.view_merge is not None:
            self.t.sync_view_radius()            # view_radius -> the device scalar the captured merge launch reads
        if self.t.scheduled:
            self.t.sync_schedule()               # ramped loss weights / teacher_alpha / mask_ratio -> the device words the captured launches read
        if self.one_graph:
            self.t.stu_optimizer.sync_hyper()    # lr scheduler / loss scale -> device state read by the captured sweep
        self.g_fb.replay()
        seg("forwards")
        if self.split:
            g = gather_activates(self.fwd_state["activates"])
            self.gathered.copy_(g if g is not None else self.fwd_state["activates"].reshape(-1))
            seg("gather")
            self.g_lb.replay()
            seg("losses+backward1")
        if self.g_lb2 is not None:
            self.t.sync.start_upper()            # suffix (94 %) on the communicator's stream ...
            self.g_lb2.replay()                  # ... under backward part 2
            seg("backward2")
            self.t.sync.finish()
            seg("finish")
        elif not self.one_graph and not self.capture_comm:
            self.t.sync()
            seg("allreduce")
        if not self.one_graph:
            self.t.stu_optimizer.sync_hyper()    # lr scheduler / loss scale -> device state read by the captured sweep
            self.g_up.replay()
            seg("update")
        self._weights_moved()
        return self.out
