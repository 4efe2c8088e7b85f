"""The drop-in boundary as the reference reaches it (train_human.py:19-29): with this package's directory first on
sys.path, the reference's own import statements resolve to the MI355X modules.  Runs the LITERAL recipe of
INTEGRATION.md (the python block after the `dropin-recipe` marker) in a fresh interpreter, from another directory."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# A stand-in for the reference checkout's host-side glue, laid out as the reference lays it out (`lib/` WITHOUT an __init__.py,
# so that _dropin.install merges it into this package's lib.__path__).  Written here, per test, so that the test needs nothing
# outside the repository; the classes are minimal stand-ins with the names the reference's scripts import.
_STAND_IN = {
    "meter.py": '''
class AverageMeter:
    def __init__(self, name, fmt=":f"):
        self.name, self.fmt = name, fmt
        self.val = self.sum = self.count = self.avg = 0.0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class AverageMeterList(AverageMeter):
    pass


class ProgressMeter:
    def __init__(self, num_batches, meters, prefix=""):
        self.num_batches, self.meters, self.prefix = num_batches, meters, prefix
''',
    "data.py": '''
class ForeverDataIterator:
    def __init__(self, loader):
        self.loader = loader
        self.it = iter(loader)

    def __next__(self):
        try:
            return next(self.it)
        except StopIteration:
            self.it = iter(self.loader)
            return next(self.it)
''',
}


def _reference_stand_in(tmp_path):
    root = tmp_path / "UDA_PoseEstimation"
    (root / "lib").mkdir(parents=True)
    for name, src in _STAND_IN.items():
        (root / "lib" / name).write_text(src)
    return str(root)


def _recipe():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"<!-- dropin-recipe -->\s*```python\n(.*?)```", text, flags=re.S)
    assert m, "INTEGRATION.md lost its dropin-recipe block"
    return m.group(1)


def _run(code, tmp_path):
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    return subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)


def test_reference_import_statements_resolve(tmp_path):
    code = _recipe().replace("/path/to/repo", ROOT)
    assert "import lib.models as models" in code and "from utils import *" in code      # the reference's own statements
    # the optional second line binds the rest of the reference's lib/ (datasets, transforms, meter ...): drop it when the
    # reference checkout is absent (GPU box); tested separately below
    code = "\n".join(l for l in code.splitlines() if "/path/to/UDA_PoseEstimation" not in l)
    code += r'''
import sys, torch
import uda_poseestimation_amd.lib.models as real_models, uda_poseestimation_amd.utils as real_utils
import uda_poseestimation_amd.lib.models.loss as real_loss, uda_poseestimation_amd.lib.keypoint_detection as real_kd
assert models is real_models and sys.modules["utils"] is real_utils, "the two spellings must be ONE module object"
assert JointsMSELoss is real_loss.JointsMSELoss and ConsLoss is real_loss.ConsLoss and accuracy is real_kd.accuracy
assert Style_net is sys.modules["uda_poseestimation_amd.lib.models.Style_net"]
assert OldWeightEMA is real_utils.OldWeightEMA and callable(rectify) and callable(get_max_preds_torch)
# train_human.py:506-510: architecture discovery
names = sorted(n for n in models.__dict__ if n.islower() and not n.startswith("__") and callable(models.__dict__[n]))
assert names == ["pose_resnet101", "pose_resnet50"], names
net = models.__dict__["pose_resnet50"](num_keypoints=16, pretrained_backbone=False)
assert sum(p.numel() for p in net.parameters()) == 36048440
opt = torch.optim.Adam(net.parameters(), lr=1e-4)
assert isinstance(Style_net.decoder, torch.nn.Sequential) and isinstance(Style_net.vgg, torch.nn.Sequential)
sn = Style_net.Net(torch.nn.Sequential(*list(Style_net.vgg.children())[:31]), Style_net.decoder)
print("DROPIN-OK")
'''
    r = _run(code, tmp_path)
    assert r.returncode == 0 and "DROPIN-OK" in r.stdout, r.stdout + r.stderr


def test_rest_of_reference_lib_still_resolves(tmp_path):
    """lib.meter / lib.data / lib.logger keep coming from the reference tree next to our lib.models (host-side glue that is
    out of scope here and imports without torchvision); the reference tree is the stand-in above."""
    reference = _reference_stand_in(tmp_path)
    code = _recipe().replace("/path/to/repo", ROOT).replace("/path/to/UDA_PoseEstimation", reference)
    code += r'''
from lib.meter import AverageMeter, ProgressMeter, AverageMeterList
from lib.data import ForeverDataIterator
import lib.meter, lib.data, os, sys
assert os.path.realpath(lib.meter.__file__).startswith(os.path.realpath("''' + reference + r'''"))
assert os.path.realpath(lib.data.__file__).startswith(os.path.realpath("''' + reference + r'''"))
assert models is sys.modules["uda_poseestimation_amd.lib.models"], "the second tree must not shadow this package's lib.models"
m = AverageMeter("x"); m.update(2.0, 4); assert m.avg == 2.0
it = ForeverDataIterator([1, 2]); assert [next(it) for _ in range(3)] == [1, 2, 1]
print("DROPIN-OK")
'''
    r = _run(code, tmp_path)
    assert r.returncode == 0 and "DROPIN-OK" in r.stdout, r.stdout + r.stderr


def test_plain_sys_path_form_without_helper(tmp_path):
    """Only the sys.path line (no _dropin call): `import lib.models` / `from utils import *` still work on their own."""
    code = f'''
import sys
sys.path.insert(0, {os.path.join(ROOT, "uda_poseestimation_amd")!r})
from utils import *
import lib.models as models
from lib.models import Style_net
from lib.keypoint_detection import accuracy
import uda_poseestimation_amd.utils as real
assert OldWeightEMA is real.OldWeightEMA and models.pose_resnet101 is not None
print("DROPIN-OK")
'''
    r = _run(code, tmp_path)
    assert r.returncode == 0 and "DROPIN-OK" in r.stdout, r.stdout + r.stderr
