"""Fused multi-tensor optimizers on MI355X kernels: drop-in torch.optim.Optimizer subclasses for the reference's
`Adam(student.parameters(), lr)` / `SGD(..., momentum=0.9, weight_decay=1e-4, nesterov=True)` (train_human.py:136-139).
One kernel launch sweeps all parameter tensors (28 B/param for Adam), instead of torch's per-group foreach chains.
In a mean-teacher step `fused_tail_step` runs either optimizer, the EMA into the teacher and both networks' weight packs as ONE
sweep (Adam 46 B/param, SGD 38), for one parameter group or for `PoseResNet.get_parameters(lr)`'s three.

Graph-replay safe: the step counter, the learning rate and the gradient scale live in an 8-float device tensor per
parameter group (`udapose_adam_multi`'s dev_state).  `sync_hyper()` uploads lr / grad_scale when the host values changed
(an lr scheduler, a loss-scale update); GraphedTrainStep calls it before every replay.  `state_dict()` is torch's plain
layout (device tables and state tensors are kept on the optimizer object, not in param_groups) with `step` read back from
the device counter; checkpoints written by torch.optim.Adam / SGD load (per-parameter `step` entries are folded into the
group counter).

Loss scaling for the fp16 precision (`dynamic_loss_scale=True`) is torch.cuda.amp.GradScaler's algorithm
(train_human.py:260,285-287) kept entirely on the device: `scale_loss(loss)` multiplies by the device-resident scale,
`step()` = found-inf sweep over the gradients -> Adam / SGD sweep that un-scales (and is skipped whole, counter included,
when an inf / nan was found) -> scale update (x backoff on overflow, x growth after `growth_interval` clean steps).
No host read-back, so the whole thing is hipGraph-capturable.

Clipping by global norm (`max_grad_norm=M`, off by default; `float("inf")` measures only) is torch.nn.utils.clip_grad_norm_'s norm and
coefficient over ALL parameter groups without rewriting a gradient: one sum-of-squares sweep per group over g (+ the pending second
per-pass buffer) in front of the first sweep - which also does the loss scaler's found-inf check, so an fp16 step reads its gradients once
- a one-work-group finisher that multiplies the coefficient into every group's device grad_scale, and a restore launch behind the sweep(s).
`grad_norm()` / `clip_coef()` are 0-d device tensors of the last step; `M` lives on the device (`sync_hyper()`), so a captured step follows
a host change.  Fixed summation order, no atomics: two runs on the same gradients give the same bits.
"""
import torch

from . import _hip
from ._hip import check, lib, ptr
from .utils import _MultiTensorTable, _bump_versions


def _norm(v):
    return tuple(v) if isinstance(v, (list, tuple)) else v


CLIP_MAX_NORM, CLIP_NORM, CLIP_COEF, CLIP_SAVED, CLIP_FLOATS = 0, 1, 2, 4, 12       # include/udapose.h UDAPOSE_CLIP_*


def _max_norm(v):
    """None (clipping off) or a positive float, +inf included (measure only)."""
    if v is None:
        return None
    v = float(v)
    if not v > 0.0:         # (NaN fails this too)
        raise ValueError(f"max_grad_norm must be None or a positive number (float('inf') measures only), got {v!r}")
    return v


def group_partition(param_groups, params):
    """The parameter-group index of every parameter of `params`, if the groups' parameters, concatenated, ARE `params` in order (what
    PoseResNet.get_parameters(lr) yields for list(net.parameters())); None for a reordered, incomplete or overlapping grouping.  Host
    only: the fused optimizer tail walks the parameters in this order and carries the index in its job table."""
    params = list(params)
    flat = [(gi, p) for gi, g in enumerate(param_groups) for p in g["params"]]
    if len(flat) != len(params) or any(a is not b for (_, a), b in zip(flat, params)):
        return None
    return [gi for gi, _ in flat]


class _FusedBase(torch.optim.Optimizer):
    _state_names = ()

    def __init__(self, params, defaults, scaler=None):
        super().__init__(params, defaults)
        self._tables = {}        # group index -> _MultiTensorTable (raw device pointers: never serialised)
        self._dev = {}           # group index -> (device state tensor [8], uploaded (lr, grad_scale))
        # dynamic loss scaling (GradScaler's defaults: 65536, x2 every 2000 clean steps, x0.5 on overflow), or None
        self._scaler = scaler
        # clipping by global norm: [UDAPOSE_CLIP_FLOATS device floats (max_norm, norm, coef, -, saved grad_scales), uploaded max_norm], and
        # one double per table block of every group; both are pointed at by captured launches and never serialised
        self._clip, self._clip_part = None, None
        self.max_grad_norm = self.defaults.get("max_grad_norm")        # (validates, and writes the one value into every group)
        if scaler is not None and len(self.param_groups) != 1:
            raise ValueError("dynamic loss scaling needs a single parameter group (one device-resident scaler state)")

    # ------------------------------------------------------------------ tables / device state
    def _gather(self, gi, group):
        ps = [p for p in group["params"] if p.grad is not None]
        if not ps:
            return None
        for p in ps:
            _hip.require_cuda(p)
            if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                raise RuntimeError("fused optimizers need fp32 parameters and gradients")
            if p.grad.stride() != p.stride():
                p.grad = p.grad.clone(memory_format=torch.preserve_format).as_strided(p.shape, p.stride()).copy_(p.grad)
            st = self.state[p]
            for n in self._state_names:
                if n not in st or not torch.is_tensor(st[n]) or st[n].device != p.device or st[n].stride() != p.stride():
                    old = st.get(n)
                    st[n] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if torch.is_tensor(old) and old.shape == p.shape:     # state loaded from a checkpoint (CPU / other layout)
                        st[n].copy_(old)
        lists = [[p.data for p in ps], [p.grad for p in ps]] + [[self.state[p][n] for p in ps] for n in self._state_names]
        key = _MultiTensorTable.key_of(lists)
        tab = self._tables.get(gi)
        if tab is None or tab.key != key:
            tab = _MultiTensorTable(lists)
            self._tables[gi] = tab
        return ps, tab

    def _dev_state(self, gi, group, device):
        """[step, bc1, bc2sqrt, lr, grad_scale, 0, 0, 0] on the device; created from the host's group values."""
        ent = self._dev.get(gi)
        if ent is None or ent[0].device != device:
            host, hyper = self._host_state(group)
            ent = [torch.tensor(host, dtype=torch.float32, device=device), hyper]
            self._dev[gi] = ent
        return ent

    def _host_state(self, group):
        """The 8 floats of a group's device state from the host's group values, and the (lr, grad_scale) pair they carry."""
        hyper = (float(group["lr"]), float(group.get("grad_scale", 1.0)))
        scale, tracker = 0.0, 0.0
        if self._scaler is not None:
            scale = float(group.get("loss_scale", self._scaler["init_scale"]))
            tracker = float(group.get("growth_tracker", 0))
            hyper = (hyper[0], 1.0 / scale)
        return [float(group.get("step", 0)), 0.0, 0.0, hyper[0], hyper[1], 0.0, scale, tracker], hyper

    # ------------------------------------------------------------------ clipping by global norm
    @property
    def max_grad_norm(self):
        """None: no clipping (no launch is added).  A positive float M: the update is scaled by min(1, M / (norm + 1e-6)), norm = the global L2
        norm of the unscaled gradient over every parameter group.  float('inf'): the norm is measured and the update is bit-identical to the
        unclipped one.  One value for the optimizer, kept in the group dicts (state_dict()); read from device memory by the kernels."""
        return self.param_groups[0].get("max_grad_norm")

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        v = _max_norm(v)
        self.defaults["max_grad_norm"] = v
        for g in self.param_groups:
            g["max_grad_norm"] = v

    def _clip_buffer(self, device):
        if self._clip is None:
            v = float(self.max_grad_norm)
            host = [0.0] * CLIP_FLOATS
            host[CLIP_MAX_NORM], host[CLIP_COEF] = v, 1.0
            self._clip = [torch.tensor(host, dtype=torch.float32, device=device), v]
        return self._clip[0]

    def grad_norm(self):
        """The global gradient norm of the last step, before clipping (clip_grad_norm_'s return value), as a 0-d DEVICE tensor; no host
        synchronisation.  None while clipping is disabled."""
        if self.max_grad_norm is None:
            return None
        return self._clip_buffer(self.param_groups[0]["params"][0].device)[CLIP_NORM]

    def clip_coef(self):
        """min(1, max_grad_norm / (norm + 1e-6)) of the last step as a 0-d DEVICE tensor; None while clipping is disabled."""
        if self.max_grad_norm is None:
            return None
        return self._clip_buffer(self.param_groups[0]["params"][0].device)[CLIP_COEF]

    def _clip_begin(self, got, ents, grad2_delta=0):
        """In front of the first sweep: the sum of squares of every group's g + g2 (with the loss scaler's found-inf check in the same read),
        then the finisher, which scales every group's device grad_scale.  got: [(params, table)] of the groups that step, ents: their device
        states.  Returns what _clip_end needs."""
        import ctypes as C
        n = len(got)
        if n > self.MAX_TAIL_GROUPS:
            raise RuntimeError(f"max_grad_norm serves at most {self.MAX_TAIL_GROUPS} parameter groups, got {n}")
        dev = ents[0][0].device
        clip = self._clip_buffer(dev)
        nblocks = sum(t.nblocks for _, t in got)
        if self._clip_part is None or self._clip_part.numel() < nblocks or self._clip_part.device != dev:
            self._clip_part = torch.empty(max(nblocks, 1), dtype=torch.float64, device=dev)
        part = self._clip_part
        begin, end, b = [], [], 0
        for (_, t), ent in zip(got, ents):
            check(lib().udapose_grad_sumsq(_hip.stream(), ptr(t.ptrs[1]), ptr(t.sizes), ptr(t.blk_t), ptr(t.blk_o), t.nblocks, int(grad2_delta),
                                           ptr(ent[0]) if self._scaler is not None else None, part.data_ptr() + 8 * b), "grad_sumsq")
            begin.append(b)
            b += t.nblocks
            end.append(b)
        states = (C.c_void_p * n)(*[e[0].data_ptr() for e in ents])
        check(lib().udapose_grad_clip(_hip.stream(), ptr(part), (C.c_int * n)(*begin), (C.c_int * n)(*end), n, states, ptr(clip)), "grad_clip")
        return n, states

    def _clip_end(self, tok):
        """Behind the last sweep (and in front of the scaler update, which refreshes 1 / S as before): every group's grad_scale back."""
        check(lib().udapose_grad_clip_restore(_hip.stream(), tok[0], tok[1], ptr(self._clip[0])), "grad_clip_restore")

    def _clip_step(self):
        """step() with clipping on: the norm over every group that has a gradient, before the first group's sweep.  Returns (token, index of
        the last such group) or None when no group has a gradient."""
        got, ents, last = [], [], None
        for gi, group in enumerate(self.param_groups):
            g = self._gather(gi, group)
            if g is not None:
                got.append(g)
                ents.append(self._dev_state(gi, group, g[0][0].device))
                last = gi
        if not got:
            return None
        self._clip_buffer(ents[0][0].device)
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        return self._clip_begin(got, ents), last

    # ------------------------------------------------------------------ loss scaling (fp16)
    def loss_scale(self):
        """The current loss scale as a 0-d DEVICE tensor (1.0 without dynamic scaling); no host synchronisation."""
        if self._scaler is None:
            return None
        p0 = self.param_groups[0]["params"][0]
        return self._dev_state(0, self.param_groups[0], p0.device)[0][6]

    def scale_loss(self, loss):
        """loss * scale (GradScaler.scale); identity without dynamic scaling."""
        sc = self.loss_scale()
        return loss if sc is None else loss * sc

    def _pre_sweep(self, t, ent, grad2_delta=0):
        """found-inf sweep of the loss scaler; grad2_delta: byte distance to a second per-pass gradient buffer whose sum is still pending
        (the fused tail adds it itself): the check then looks at g + g2."""
        if self._scaler is not None and self.max_grad_norm is None:        # (with clipping the sum-of-squares sweep has checked already)
            check(lib().udapose_grad_scaler_check2(_hip.stream(), ptr(t.ptrs[1]), ptr(t.sizes), ptr(t.blk_t), ptr(t.blk_o), t.nblocks, ptr(ent[0]),
                                                   int(grad2_delta)), "grad_scaler_check")

    def _post_sweep(self, ent):
        if self._scaler is not None:
            sc = self._scaler
            check(lib().udapose_grad_scaler_update(_hip.stream(), ptr(ent[0]), float(sc["growth_factor"]), float(sc["backoff_factor"]),
                                                   int(sc["growth_interval"])), "grad_scaler_update")

    def sync_hyper(self):
        """Upload lr / grad_scale of every group whose host value changed since the last upload (stream-ordered 8-byte copy;
        call before replaying a captured step); likewise max_grad_norm."""
        if self._clip is not None and self.max_grad_norm is not None and float(self.max_grad_norm) != self._clip[1]:
            v = float(self.max_grad_norm)
            self._clip[0][CLIP_MAX_NORM:CLIP_MAX_NORM + 1].copy_(torch.tensor([v], dtype=torch.float32), non_blocking=True)
            self._clip[1] = v
        for gi, group in enumerate(self.param_groups):
            ent = self._dev.get(gi)
            if ent is None:
                continue
            if self._scaler is not None:           # grad_scale = 1 / loss scale is owned by the device-side scaler
                if float(group["lr"]) != ent[1][0]:
                    ent[0][3:4].copy_(torch.tensor([float(group["lr"])], dtype=torch.float32), non_blocking=True)
                    ent[1] = (float(group["lr"]), ent[1][1])
                continue
            hyper = (float(group["lr"]), float(group.get("grad_scale", 1.0)))
            if hyper != ent[1]:
                ent[0][3:5].copy_(torch.tensor(hyper, dtype=torch.float32), non_blocking=True)
                ent[1] = hyper

    # ------------------------------------------------------------------ fused tail: optimizer + EMA + weight packs in one sweep
    _tail_kind = None               # the library's optimizer kind (include/udapose.h UDAPOSE_OPT_*); None: no fused tail
    _tail_agree = ()                # hyper-parameters the sweep takes by value once: they must agree across the groups
    tail_takes_split_sums = False
    MAX_TAIL_GROUPS = 8

    def fused_tail_step(self, student, teacher, ema):
        """One launch for the optimizer step on the student (torch.optim.Adam / SGD with momentum), OldWeightEMA.step into the teacher
        and the weight packs of the two executor plans their last forwards used (udapose_net_fused_update_groups).  Several parameter
        groups are served when, concatenated, they are list(student.parameters()) in order (PoseResNet.get_parameters) and agree on
        everything but lr and weight_decay.  Returns False - nothing done - when the layout is not the one the kernel serves (then
        step() and ema.step() apply)."""
        import ctypes as C
        if self._tail_kind is None or not 1 <= len(self.param_groups) <= self.MAX_TAIL_GROUPS:
            return False
        groups = self.param_groups
        if any(_norm(g[k]) != _norm(groups[0][k]) for g in groups[1:] for k in self._tail_agree):
            return False
        ps = list(student.parameters())
        hd_s, hd_t = getattr(student, "_last_hd", None), getattr(teacher, "_last_hd", None)
        # the teacher either shares the student's 16-bit element type (its packs are written by the sweep) or runs the fp32-grade
        # f16x2 mode (the reference's precision mix: its split packs are refreshed by one pack launch right after the sweep)
        # (a 'strict' student - f16x2 forward, fp16 backward, fp16 build - gets its fp16 data-gradient packs from the sweep and its split
        # forward packs from one pack launch inside udapose_net_fused_update)
        if hd_s is None or hd_t is None or hd_s.precision not in ("bf16", "fp16", "strict"):
            return False
        s_kind = "fp16" if hd_s.precision == "strict" else hd_s.precision      # (the student's library build)
        t_split = hd_t.precision == "f16x2"
        # both plans are handed to ONE library (the student's): the teacher's must have been created by it (PoseResNet.aux_lib_kind puts an
        # f16x2 teacher's plan into the student's build; a plan of the other .so is never dereferenced here - ADVICE r3)
        if hd_s.L is not hd_t.L and t_split and hasattr(teacher, "aux_lib_kind") and teacher.aux_lib_kind != s_kind:
            # an 'auto' student resolved to the other build than the one the teacher's f16x2 plan was created in (the engine guesses the
            # build before the first forward): move the teacher's fp32-grade plans into the student's build - the next teacher forward
            # creates its plan there, and the one-launch tail applies from the following step on
            teacher.aux_lib_kind = s_kind
        if hd_s.L is not hd_t.L or (not t_split and hd_t.precision != hd_s.precision) or (hd_s.precision == "strict" and not t_split):
            if not getattr(self, "_warned_tail_lib", False):
                self._warned_tail_lib = True
                import warnings
                warnings.warn("fused optimizer tail refused: the student's and the teacher's plans live in different library builds "
                              f"({hd_s.precision} / {hd_t.precision}); falling back to separate optimizer + EMA + pack launches for this step")
            return False
        part = group_partition(groups, ps)
        if part is None:
            return False
        if len(ema.source_params) != len(ps) or any(a is not b for a, b in zip(ema.source_params, ps)):
            return False
        got = [self._gather(gi, group) for gi, group in enumerate(groups)]
        if any(g is None for g in got):         # (a group without any gradient: step() would leave its counter alone)
            return False
        with_grad = [p for g in got for p in g[0]]
        ents = [self._dev_state(gi, group, ps[0].device) for gi, group in enumerate(groups)]
        tps = ema.target_params
        names = self._state_names
        key = (ps[0].data_ptr(), tps[0].data_ptr(), with_grad[0].grad.data_ptr(), self.state[with_grad[0]][names[0]].data_ptr(),
               hd_s.wpack.data_ptr(), hd_t.wpack.data_ptr(), len(with_grad), tuple(part), tuple(e[0].data_ptr() for e in ents))
        cache = getattr(self, "_tail", None)
        if cache is None or cache[0] != key:
            n = len(ps)
            arr = lambda vals: (C.c_void_p * n)(*vals)
            st = [self.state[p] if p.grad is not None else None for p in ps]
            cache = (key, arr([p.data_ptr() for p in ps]), arr([p.grad.data_ptr() if p.grad is not None else None for p in ps]),
                     arr([s_[names[0]].data_ptr() if s_ else None for s_ in st]),
                     arr([s_[names[1]].data_ptr() if s_ else None for s_ in st]) if len(names) > 1 else None,
                     arr([p.data_ptr() for p in tps]), (C.c_int * n)(*part), (C.c_void_p * len(ents))(*[e[0].data_ptr() for e in ents]))
            rc = hd_s.L.udapose_net_bind_update_groups(hd_s.h, hd_t.h, self._tail_kind, cache[1], cache[2], cache[3], cache[4], cache[5],
                                                       ptr(hd_s.wpack), ptr(hd_t.wpack), cache[6])
            if rc == -3:        # unsupported layout (unaligned tensors, channel counts that are not multiples of 64)
                self._tail = None
                return False
            check(rc, "net_bind_update_groups")
            self._tail = cache
        _, pa_s, ga, ma, va, pa_t, _, states = cache
        for group in groups:
            group["step"] = group.get("step", 0) + 1
        clipping = self.max_grad_norm is not None
        if clipping:
            self._clip_buffer(ps[0].device)
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        # a pending sum of the two passes' gradient buffers is taken in the sweep itself (no separate axpy over 220 MB) - and by the loss
        # scaler's inf / nan check in front of it, which looks at g + g2 (round 4: the fp16 step used to force the sum first)
        delta = student.pending_grad_sum(take=True) if hasattr(student, "pending_grad_sum") else 0
        # clipping: the norm of g + g2 over every group (and the found-inf check) in front of the sweep, the grad_scales back behind it
        clip = self._clip_begin(got, ents, delta) if clipping else None
        self._pre_sweep(got[0][1], ents[0], delta)         # (loss scaling: one group)
        b1, b2, eps, nesterov = self._tail_hyper(groups[0])
        wds = (C.c_float * len(groups))(*[float(g["weight_decay"]) for g in groups])
        ema_dev = getattr(ema, "alpha_dev", None)
        if ema_dev is not None:         # (a scheduled teacher_alpha: the sweep reads {alpha, 1 - alpha} from device memory - the same two fp32 values)
            check(hd_s.L.udapose_net_fused_update_groups_dev(hd_s.h, hd_t.h, _hip.stream(), self._tail_kind, pa_s, ga, ma, pa_t, ptr(hd_s.wpack),
                                                             ptr(hd_t.wpack), b1, b2, eps, nesterov, len(groups), states, wds, ptr(ema_dev), 1,
                                                             int(delta)), "net_fused_update_groups_dev")
        else:
            check(hd_s.L.udapose_net_fused_update_groups(hd_s.h, hd_t.h, _hip.stream(), self._tail_kind, pa_s, ga, ma, pa_t, ptr(hd_s.wpack),
                                                         ptr(hd_t.wpack), b1, b2, eps, nesterov, len(groups), states, wds, float(ema.alpha),
                                                         float(1.0 - ema.alpha), 1, int(delta)), "net_fused_update_groups")
        if clip is not None:
            self._clip_end(clip)
        return self._tail_finish(student, teacher, hd_s, hd_t, ps, tps, t_split, ents[0])

    def _tail_finish(self, student, teacher, hd_s, hd_t, ps, tps, t_split, ent):
        self._post_sweep(ent)
        _bump_versions(ps)
        _bump_versions(tps)
        student.packs_refreshed(hd_s, True)
        if t_split:
            pa_t_ = teacher._pointers()[0]
            check(hd_t.L.udapose_net_pack_weights(hd_t.h, _hip.stream(), pa_t_, ptr(hd_t.wpack), 0), "net_pack_weights (teacher, f16x2)")
        teacher.packs_refreshed(hd_t, False)
        return True

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        for gi, group in enumerate(self.param_groups):
            ent = self._dev.get(gi)
            if ent is not None:
                host = ent[0].tolist()
                group["step"] = int(round(host[0]))                       # replays tick the device counter only
                if self._scaler is not None:
                    group["loss_scale"], group["growth_tracker"] = float(host[6]), int(round(host[7]))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """torch's load, then (1) the group step counter from wherever the checkpoint keeps it, (2) IN PLACE: moment / momentum tensors
        and device state that already exist keep their storage and receive the loaded values, so kernels captured in a hipGraph
        (GraphedTrainStep), which hold raw pointers to them, go on working on the restored state."""
        old_state = {p: dict(st) for p, st in self.state.items()}
        old_dev = dict(self._dev)
        max_norm = self.max_grad_norm
        super().load_state_dict(state_dict)
        for group in self.param_groups:             # (a checkpoint from before max_grad_norm existed keeps the current setting)
            group.setdefault("max_grad_norm", max_norm)
        self.max_grad_norm = self.param_groups[0]["max_grad_norm"]
        for group in self.param_groups:
            if "step" not in group or group["step"] is None:
                # torch.optim.Adam / SGD checkpoints keep `step` per parameter (or not at all)
                steps = [float(self.state[p]["step"]) for p in group["params"] if p in self.state and "step" in self.state[p]]
                group["step"] = int(max(steps)) if steps else 0
                if not steps and any(torch.is_tensor(self.state.get(p, {}).get("momentum_buffer")) for p in group["params"]):
                    # torch.optim.SGD keeps no step at all: restored momentum buffers mean "not the first step" (the first step
                    # INITIALISES the buffer with the gradient, train_human.py:136,157,231 resume SGD runs from such checkpoints)
                    group["step"] = 1
            group.setdefault("grad_scale", 1.0)
        for p, st in self.state.items():
            o = old_state.get(p)
            if not o:
                continue
            for n in self._state_names:
                a, b = o.get(n), st.get(n)
                if torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and a.device == p.device and a.stride() == p.stride():
                    a.copy_(b)
                    st[n] = a
        self._dev = {}
        for gi, group in enumerate(self.param_groups):
            ent = old_dev.get(gi)
            if ent is not None:
                host, hyper = self._host_state(group)
                ent[0].copy_(torch.tensor(host, dtype=torch.float32))
                ent[1] = hyper
                self._dev[gi] = ent
        # (job tables are keyed by the tensors' pointers: they stay valid where the storage was kept, and are rebuilt otherwise)


class FusedAdam(_FusedBase):
    _state_names = ("exp_avg", "exp_avg_sq")
    _tail_kind = 0                              # UDAPOSE_OPT_ADAM
    _tail_agree = ("betas", "eps")
    tail_takes_split_sums = True                # (the sweep that adds the split weight-gradient sums itself exists for Adam only)

    @staticmethod
    def _tail_hyper(group):
        b1, b2 = group["betas"]
        return float(b1), float(b2), float(group["eps"]), 0

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, dynamic_loss_scale=False,
                 init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, max_grad_norm=None):
        scaler = dict(init_scale=init_scale, growth_factor=growth_factor, backoff_factor=backoff_factor,
                      growth_interval=growth_interval) if dynamic_loss_scale else None
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, step=0,
                                      max_grad_norm=_max_norm(max_grad_norm)), scaler)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        capturing = torch.cuda.is_current_stream_capturing()
        clip = self._clip_step() if self.max_grad_norm is not None else None       # (the norm over every group, before the first sweep)
        for gi, group in enumerate(self.param_groups):
            got = self._gather(gi, group)
            if got is None:
                continue
            ps, t = got
            ent = self._dev_state(gi, group, ps[0].device)          # (created with the number of steps done so far)
            group["step"] = group.get("step", 0) + 1
            b1, b2 = group["betas"]
            if not capturing:
                self.sync_hyper()
            self._pre_sweep(t, ent)
            check(lib().udapose_adam_multi(_hip.stream(), ptr(t.ptrs[0]), ptr(t.ptrs[1]), ptr(t.ptrs[2]), ptr(t.ptrs[3]), ptr(t.sizes), ptr(t.blk_t),
                                           ptr(t.blk_o), t.nblocks, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                           float(group["weight_decay"]), int(group["step"]), float(group.get("grad_scale", 1.0)), ptr(ent[0])),
                  "adam_multi")
            if clip is not None and gi == clip[1]:
                self._clip_end(clip[0])
            self._post_sweep(ent)
            _bump_versions(ps)
        return loss


class FusedSGD(_FusedBase):
    _state_names = ("momentum_buffer",)
    _tail_kind = 1                              # UDAPOSE_OPT_SGD
    _tail_agree = ("momentum", "nesterov")

    @staticmethod
    def _tail_hyper(group):
        return float(group["momentum"]), 0.0, 0.0, int(bool(group["nesterov"]))

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, nesterov=False, grad_scale=1.0, dynamic_loss_scale=False,
                 init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, max_grad_norm=None):
        scaler = dict(init_scale=init_scale, growth_factor=growth_factor, backoff_factor=backoff_factor,
                      growth_interval=growth_interval) if dynamic_loss_scale else None
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov, grad_scale=grad_scale, step=0,
                                      max_grad_norm=_max_norm(max_grad_norm)), scaler)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        capturing = torch.cuda.is_current_stream_capturing()
        clip = self._clip_step() if self.max_grad_norm is not None else None       # (the norm over every group, before the first sweep)
        for gi, group in enumerate(self.param_groups):
            got = self._gather(gi, group)
            if got is None:
                continue
            ps, t = got
            ent = self._dev_state(gi, group, ps[0].device)
            group["step"] = group.get("step", 0) + 1
            if not capturing:
                self.sync_hyper()
            self._pre_sweep(t, ent)
            check(lib().udapose_sgd_multi(_hip.stream(), ptr(t.ptrs[0]), ptr(t.ptrs[1]), ptr(t.ptrs[2]), ptr(t.sizes), ptr(t.blk_t), ptr(t.blk_o),
                                          t.nblocks, float(group["lr"]), float(group["momentum"]), float(group["weight_decay"]),
                                          int(group["nesterov"]), int(group["step"] == 1), float(group.get("grad_scale", 1.0)), ptr(ent[0])),
                  "sgd_multi")
            if clip is not None and gi == clip[1]:
                self._clip_end(clip[0])
            self._post_sweep(ent)
            _bump_versions(ps)
        return loss
