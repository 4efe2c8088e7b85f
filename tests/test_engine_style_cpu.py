"""The engine's style-net adapter and its reset methods, the part that needs no GPU: stub style nets, one per protocol, record what the
eager style pass (MeanTeacherTrainer._style_part) and the captured one (GraphedTrainStep._style_pass) ask of them; a net with the plain call
only is refused by GraphedTrainStep before it touches a tensor; GradSync.reset() and PoseResNet._drop_pending_step() restore constructor
values; engine.py assigns to no private field of the gradient exchange or of a network."""
import inspect
import itertools
import re

import pytest
import torch

from uda_poseestimation_amd import engine
from uda_poseestimation_amd.engine import GradSync, GraphedTrainStep, MeanTeacherTrainer

RECOVER = object()          # the trainer's clamp argument: handed through untouched


class _Stub:
    """Records ("summarize", image, result) and ("transfer", content image | None, content summary, style summary, alpha, clamp, result);
    every result is a fresh CPU tensor that carries the call's number."""

    def __init__(self):
        self.calls = []

    def _tag(self, shape=(1,)):
        return torch.full(shape, float(len(self.calls)))

    def _ret(self, value, out):
        return value if out is None else out.copy_(value)


class FdaStub(_Stub):
    def spectrum(self, img, out=None):
        r = self._ret(self._tag(), out)
        self.calls.append(("summarize", img, r))
        return r

    def transfer(self, content, spec_content, spec_style, alpha=1.0, clamp=None, out=None):
        r = self._ret(self._tag(), out)
        self.calls.append(("transfer", content, spec_content, spec_style, alpha, clamp, r))
        return r


class AdainStub(_Stub):
    compute_losses = False

    def encode_features(self, img):
        r = self._tag()
        self.calls.append(("summarize", img, r))
        return r

    def transfer_from_features(self, content_feat, style_feat, alpha=1.0, clamp=None):
        r = self._tag()
        self.calls.append(("transfer", None, content_feat, style_feat, alpha, clamp, r))
        return r

    def __call__(self, content, style, alpha=1.0, clamp=None):
        r = self._tag()
        self.calls.append(("transfer", None, content, style, alpha, clamp, r))
        return None, None, r


class PlainStub(_Stub):
    def __call__(self, content, style, alpha=1.0, clamp=None):
        r = self._tag()
        self.calls.append(("transfer", None, content, style, alpha, clamp, r))
        return None, None, r


class _Draws:
    """rand() / uniform() in the order draw_style_decisions asks: a direction is drawn when its rand() is below the frequency 0.5."""

    def __init__(self, s2t, t2s):
        self.rands = [0.0 if s2t else 1.0, 0.0 if t2s else 1.0]
        self.alphas = [0.25, 0.75]

    def rand(self):
        return self.rands.pop(0)

    def uniform(self, lo, hi):
        return self.alphas[0 if len(self.rands) == 1 else 1]        # (s2t's alpha is drawn before t2s's rand)


def _trainer(net, s2t=False, t2s=False):
    tr = MeanTeacherTrainer.__new__(MeanTeacherTrainer)
    tr.style_net, tr.recover, tr.rng = net, RECOVER, _Draws(s2t, t2s)
    tr._style = engine._StyleAdapter(net)
    tr.s2t_freq = tr.t2s_freq = 0.5
    tr.s2t_alpha = tr.t2s_alpha = (0.0, 1.0)
    return tr


def _same(a, b):
    return len(a) == len(b) and all(x is y for x, y in zip(a, b))


def _check_style_part(net, form, views, s2t, t2s):
    x_s, x_ts = torch.zeros(1), [torch.zeros(1) for _ in range(views)]
    out_s, out_ts = _trainer(net, s2t, t2s)._style_part(x_s, list(x_ts))
    sums = [c for c in net.calls if c[0] == "summarize"]
    trans = [c for c in net.calls if c[0] == "transfer"]
    assert len(sums) + len(trans) == len(net.calls)
    if not (s2t or t2s):
        assert net.calls == [] and out_s is x_s and _same(out_ts, x_ts)
        return
    # each image summarised at most once, from the ORIGINAL; without t2s only the first teacher view
    want_summarised = [] if form == "plain" else [x_s] + (x_ts if t2s else x_ts[:1])
    assert _same([c[1] for c in sums], want_summarised)
    assert net.calls[:len(sums)] == sums                      # (all summaries before the first transfer)

    def summary(img):
        return img if form == "plain" else next(c[2] for c in sums if c[1] is img)

    want = ([(x_s, summary(x_s), summary(x_ts[0]), 0.25)] if s2t else []) + \
           ([(x_t, summary(x_t), summary(x_s), 0.75) for x_t in x_ts] if t2s else [])
    assert len(trans) == len(want)
    for got, (img, sc, ss, alpha) in zip(trans, want):
        assert got[2] is sc and got[3] is ss and got[4] == alpha and got[5] is RECOVER
        assert got[1] is (img if form == "fda" else None)
    results = [c[6] for c in trans]
    assert out_s is (results[0] if s2t else x_s)
    assert _same(out_ts, results[1 if s2t else 0:] if t2s else x_ts)


@pytest.mark.parametrize("views", [1, 2])
@pytest.mark.parametrize("s2t,t2s", list(itertools.product([False, True], repeat=2)))
@pytest.mark.parametrize("form", ["fda", "adain", "plain"])
def test_style_part_summarises_once_and_transfers_from_the_originals(form, s2t, t2s, views):
    net = {"fda": FdaStub, "adain": AdainStub, "plain": PlainStub}[form]()
    assert engine._StyleAdapter(net).form == form
    _check_style_part(net, form, views, s2t, t2s)


@pytest.mark.parametrize("views", [1, 2])
def test_style_part_takes_the_plain_call_when_the_net_computes_losses(views):
    net = AdainStub()
    net.compute_losses = True
    _check_style_part(net, "plain", views, True, True)
    assert engine._StyleAdapter(net, captured=True).form == "adain"       # (the captured pass ignores the flag)


def test_a_data_parallel_wrap_is_unwrapped_for_the_fast_protocols_only():
    class Wrap:
        def __init__(self, module):
            self.module, self.called = module, 0

        def __call__(self, *a, **k):
            self.called += 1
            return self.module(*a, **k)

    w = Wrap(FdaStub())
    _trainer(w, True, False)._style_part(torch.zeros(1), [torch.zeros(1)])
    assert w.called == 0 and [c[0] for c in w.module.calls] == ["summarize", "summarize", "transfer"]
    w = Wrap(PlainStub())
    _trainer(w, True, False)._style_part(torch.zeros(1), [torch.zeros(1)])
    assert w.called == 1                                                    # the reference's call goes to the object it was given


@pytest.mark.parametrize("form", ["fda", "adain"])
def test_captured_style_pass_fills_static_buffers_through_the_adapter(form):
    net = {"fda": FdaStub, "adain": AdainStub}[form]()
    gs = GraphedTrainStep.__new__(GraphedTrainStep)
    gs.t, gs._style, gs.g_style = _trainer(net), engine._StyleAdapter(net, captured=True), {}
    st = gs.static = {"x_s": torch.zeros(1), "x_t_tea": torch.zeros(1), "x_s_in": torch.zeros(1), "x_t_tea_in": torch.zeros(1),
                      "alpha_s2t": torch.ones(1), "alpha_t2s": torch.ones(1)}
    k_s, k_t = {"fda": ("sp_s", "sp_t"), "adain": ("f_s", "f_t")}[form]
    gs._style_pass("enc")
    assert _same([c[1] for c in net.calls], [st["x_s"], st["x_t_tea"]])
    assert float(st[k_s]) == 0.0 and float(st[k_t]) == 1.0
    assert st[k_s] is not net.calls[0][2] and st[k_t] is not net.calls[1][2]         # buffers of the step's own
    buf_s, buf_t = st[k_s], st[k_t]
    gs._style_pass("enc")                                                           # the captured form: into the same buffers
    assert st[k_s] is buf_s and st[k_t] is buf_t and float(buf_s) == 2.0 and float(buf_t) == 3.0
    gs._style_pass("s2t")
    gs._style_pass("t2s")
    s2t, t2s = net.calls[4], net.calls[5]
    assert s2t[2] is buf_s and s2t[3] is buf_t and s2t[4] is st["alpha_s2t"] and s2t[5] is RECOVER
    assert t2s[2] is buf_t and t2s[3] is buf_s and t2s[4] is st["alpha_t2s"] and t2s[5] is RECOVER
    assert s2t[1] is (st["x_s"] if form == "fda" else None) and t2s[1] is (st["x_t_tea"] if form == "fda" else None)
    assert float(st["x_s_in"]) == 4.0 and float(st["x_t_tea_in"]) == 5.0
    assert len(net.calls) == 6


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"GraphedTrainStep touched an argument (.{name}) before refusing the style net")


@pytest.mark.parametrize("args", [tuple(torch.zeros(2, 3) for _ in range(7)), tuple(_Untouchable() for _ in range(7))],
                         ids=["cpu_tensors", "untouchable"])
def test_graphed_step_refuses_a_plain_only_style_net_first(args, monkeypatch):
    def no_clone(self, *a, **k):
        raise AssertionError("GraphedTrainStep cloned a tensor before refusing the style net")

    monkeypatch.setattr(torch.Tensor, "clone", no_clone)
    net = PlainStub()
    with pytest.raises(TypeError) as e:
        GraphedTrainStep(_trainer(net), *args)
    msg = str(e.value)
    assert "spectrum" in msg and "transfer" in msg and "encode_features" in msg and "transfer_from_features" in msg
    assert net.calls == []


def test_owners_reset_their_per_step_state():
    import uda_poseestimation_amd.lib.models.pose_resnet as pr

    class M:
        pass
    sync = GradSync(M())
    fresh = (sync._work, sync._upper, sync._cstream)
    assert fresh == (None, None, None)
    sync._work, sync._upper, sync._cstream = "stream", torch.zeros(3), object()
    sync.reset()
    assert (sync._work, sync._upper, sync._cstream) == fresh
    net = pr._pose_resnet("t", 16, pr.Bottleneck_default, [1, 1, 1, 1], False, False)
    assert (net._pending_lower, net._pending_wg, net._grad_state) == ([], [], None)
    handles = net._handles
    net._pending_lower, net._pending_wg, net._grad_state = [1], [2], [None, True]
    net._drop_pending_step()
    assert (net._pending_lower, net._pending_wg, net._grad_state) == ([], [], None)
    assert net._handles is handles                                                  # (only the per-step work)
    net._pending_lower, net._pending_wg, net._grad_state = [1], [2], [None, True]
    net.float()                                                                     # _apply drops it too, with the rest
    assert (net._pending_lower, net._pending_wg, net._grad_state) == ([], [], None) and net._handles is not handles


def test_engine_assigns_to_no_private_field_of_the_exchange_or_the_networks():
    src = inspect.getsource(engine)
    assign = re.compile(r"^(?P<lhs>[^=\n]*?[^=!<>\s])\s*=(?!=)", re.M)
    for m in assign.finditer(src):
        lhs = m.group("lhs").split("#")[0]
        assert not re.search(r"\.sync\._\w", lhs), lhs
        assert not re.search(r"\._pending_\w|\._grad_state", lhs), lhs
    assert "hasattr" not in inspect.getsource(MeanTeacherTrainer._style_part) + inspect.getsource(GraphedTrainStep._style_pass)
