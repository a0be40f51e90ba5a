"""TEST INFRASTRUCTURE ONLY - stand-ins for the handful of torchvision functions that the reference's ``datasets/transforms.py`` and
``datasets/coco.py`` call on PIL images, written here over Pillow (12.2 in this image; torchvision itself is absent), on top of the
package stubs of ``oracle/ref_shims.py``:

  * ``torchvision.transforms.functional.resize(img, (h, w))``  = ``img.resize((w, h), PIL.Image.BILINEAR)`` (torchvision's default
    interpolation, and what it does for a PIL image and a two-element size)
  * ``functional.crop(img, top, left, height, width)``         = ``img.crop((left, top, left + width, top + height))``
  * ``functional.hflip(img)``                                  = ``img.transpose(PIL.Image.FLIP_LEFT_RIGHT)``
  * ``functional.to_tensor(img)``                              = uint8 HWC -> CHW, ``.to(float32).div(255)``
  * ``functional.normalize(t, mean, std)``                     = ``(t - mean[:, None, None]) / std[:, None, None]`` in ``t``'s dtype
  * ``transforms.RandomCrop.get_params(img, (th, tw))``        = torchvision's draw order: nothing when the crop is the whole image,
    else ``torch.randint(0, h - th + 1, (1,))`` for the top, then ``torch.randint(0, w - tw + 1, (1,))`` for the left
  * ``torchvision.datasets.CocoDetection``                     = an empty base class (``datasets/coco.py`` derives from it on import)

``tools/gen_golden_augment.py`` imports the reference's transforms through these and writes ``tests/golden/augment.npz``: those goldens
are the reference transforms over real Pillow through these stand-ins. The pixel arithmetic under test - the resampler - is Pillow's
own; the stand-ins only route the reference's calls to it. No test imports this module: the tests read the fixture."""
import importlib
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_shims  # noqa: E402


def resize(img, size, interpolation=None, max_size=None, antialias=None):
    if not isinstance(size, (list, tuple)) or len(size) != 2:
        raise TypeError("the stand-in takes a (h, w) size, which is all the reference passes")
    return img.resize((int(size[1]), int(size[0])), Image.BILINEAR)


def crop(img, top, left, height, width):
    return img.crop((left, top, left + width, top + height))


def hflip(img):
    return img.transpose(Image.FLIP_LEFT_RIGHT)


def to_tensor(pic):
    img = torch.from_numpy(np.array(pic, np.uint8, copy=True))
    img = img.view(pic.size[1], pic.size[0], len(pic.getbands())).permute((2, 0, 1)).contiguous()
    return img.to(dtype=torch.float32).div(255)


def normalize(tensor, mean, std, inplace=False):
    if not inplace:
        tensor = tensor.clone()
    mean = torch.as_tensor(mean, dtype=tensor.dtype, device=tensor.device).view(-1, 1, 1)
    std = torch.as_tensor(std, dtype=tensor.dtype, device=tensor.device).view(-1, 1, 1)
    return tensor.sub_(mean).div_(std)


class RandomCrop:
    @staticmethod
    def get_params(img, output_size):
        w, h = img.size
        th, tw = output_size
        if h < th or w < tw:
            raise ValueError(f"Required crop size {(th, tw)} is larger than input image size {(h, w)}")
        if w == tw and h == th:
            return 0, 0, h, w
        i = torch.randint(0, h - th + 1, size=(1,)).item()
        j = torch.randint(0, w - tw + 1, size=(1,)).item()
        return i, j, th, tw


def install():
    """Registers the stand-ins; returns (datasets.transforms, datasets.coco) of the reference, imported through them."""
    if not ref_shims.reference_available():
        raise RuntimeError(f"{ref_shims.REFERENCE_ROOT} is not present")
    ref_shims._install_shims()
    tv = sys.modules["torchvision"]
    tt = types.ModuleType("torchvision.transforms")
    tf = types.ModuleType("torchvision.transforms.functional")
    tf.resize, tf.crop, tf.hflip, tf.to_tensor, tf.normalize = resize, crop, hflip, to_tensor, normalize
    tt.RandomCrop, tt.functional = RandomCrop, tf
    td = types.ModuleType("torchvision.datasets")
    td.CocoDetection = type("CocoDetection", (object,), {})
    tv.transforms, tv.datasets = tt, td
    sys.modules.update({"torchvision.transforms": tt, "torchvision.transforms.functional": tf, "torchvision.datasets": td})
    if ref_shims.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_shims.REFERENCE_ROOT)
    if "datasets" not in sys.modules:            # the package without its __init__ (which pulls in the dataset classes' dependencies)
        pkg = types.ModuleType("datasets")
        pkg.__path__ = [os.path.join(ref_shims.REFERENCE_ROOT, "datasets")]
        sys.modules["datasets"] = pkg
    return importlib.import_module("datasets.transforms"), importlib.import_module("datasets.coco")
