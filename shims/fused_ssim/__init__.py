"""Shadow of the third-party CUDA extension `fused_ssim` (the reference's requirements_extra.txt:2): with `<repo>/shims` on PYTHONPATH,
`threedgrut/model/losses.py:17` (`from fused_ssim import fused_ssim`) binds to the MI355X fused SSIM of 3dgrut_amd/losses.py unchanged."""
import importlib as _il
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)
fused_ssim = _il.import_module("3dgrut_amd.losses").fused_ssim

__all__ = ["fused_ssim"]
