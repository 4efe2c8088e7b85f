"""Host side of the grouped optimizer tail (no GPU): the interface exists, and the group-partition check that decides whether a
multi-group optimizer may take the one-sweep tail accepts PoseResNet.get_parameters() and nothing that is reordered or incomplete."""
import inspect

import torch


def _net(finetune=True):
    import uda_poseestimation_amd.lib.models.pose_resnet as pr
    torch.manual_seed(0)
    return pr._pose_resnet("t", 16, pr.Bottleneck_default, [1, 1, 1, 1], False, False, finetune)


def test_interface_exists():
    from uda_poseestimation_amd import _hip, optim as fo
    from uda_poseestimation_amd.engine import MeanTeacherTrainer
    assert callable(getattr(fo.FusedSGD, "fused_tail_step", None)) and callable(getattr(fo.FusedAdam, "fused_tail_step", None))
    assert fo.FusedSGD.fused_tail_step is fo.FusedAdam.fused_tail_step          # one implementation, in the base class
    assert fo.FusedAdam.tail_takes_split_sums and not fo.FusedSGD.tail_takes_split_sums
    sig = inspect.signature(MeanTeacherTrainer.__init__)
    assert "params" in sig.parameters and sig.parameters["params"].default is None
    assert {"udapose_net_bind_update_groups", "udapose_net_fused_update_groups", "udapose_net_bind_update", "udapose_net_fused_update"} <= set(_hip.EXPORTS)


def test_group_partition_accepts_get_parameters():
    from uda_poseestimation_amd import optim as fo
    net = _net()
    for opt in (fo.FusedSGD(net.get_parameters(1e-3), lr=1e-3, momentum=0.9, nesterov=True), fo.FusedAdam(net.get_parameters(1e-3))):
        assert [g["lr"] for g in opt.param_groups] == [1e-4, 1e-3, 1e-3]
        part = fo.group_partition(opt.param_groups, net.parameters())
        params = list(net.parameters())
        assert part is not None and len(part) == len(params)
        assert part == sorted(part) and set(part) == {0, 1, 2}
        assert part.count(0) == len(list(net.backbone.parameters())) and part.count(2) == len(list(net.head.parameters()))
    one = fo.FusedAdam(net.parameters())
    assert fo.group_partition(one.param_groups, net.parameters()) == [0] * len(list(net.parameters()))


def test_group_partition_rejects_reordered_and_incomplete_groupings():
    from uda_poseestimation_amd import optim as fo
    net = _net()
    params = list(net.parameters())
    g = [dict(params=list(d["params"])) for d in net.get_parameters(1e-3)]
    assert fo.group_partition(g, params) is not None
    assert fo.group_partition([g[1], g[0], g[2]], params) is None               # groups in another order
    assert fo.group_partition(g[:2], params) is None                            # the head is missing
    assert fo.group_partition([g[0], g[1], g[2], dict(params=[params[0]])], params) is None     # a parameter twice
    swapped = list(g[0]["params"])
    swapped[0], swapped[1] = swapped[1], swapped[0]
    assert fo.group_partition([dict(params=swapped), g[1], g[2]], params) is None               # reordered inside a group
    other = _net()
    assert fo.group_partition(g, other.parameters()) is None                    # another network's parameters
