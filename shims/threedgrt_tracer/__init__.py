"""Shadow of the reference's `threedgrt_tracer` package (see shims/threedgut_tracer/__init__.py):
`threedgrut/model/model.py:23` (`import threedgrt_tracer`) binds to the MI355X software-BVH tracer."""
import importlib as _il
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)
Tracer = _il.import_module("3dgrut_amd.grt_tracer").Tracer
# the MCMC strategy's plugin (threedgrut/strategy/mcmc.py:41 `from . import lib_mcmc_cc`): registered before any strategy exists
_il.import_module("3dgrut_amd.mcmc").install()
# the loss's extension (threedgrut/model/losses.py:17 `from fused_ssim import fused_ssim`): the HIP fused SSIM unless one is installed
_il.import_module("3dgrut_amd.losses").install()
# the post-processing package (threedgrut/trainer.py:470 `from ppisp import PPISP, PPISPConfig`): the HIP PPISP unless one is installed
_il.import_module("3dgrut_amd.ppisp").install()
# the NHT decoder's network (threedgrut/model/feature_decoder.py:16 `import tinycudann as tcnn`): the HIP MLP unless one is installed
_il.import_module("3dgrut_amd.tcnn").install()

__all__ = ["Tracer"]
