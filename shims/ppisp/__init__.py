"""Shadow of the third-party CUDA package `ppisp` (the reference's post_processing.method: ppisp): with `<repo>/shims` on PYTHONPATH,
`threedgrut/trainer.py:470` (`from ppisp import PPISP, PPISPConfig`), `threedgrut/render.py:138` and the exporter's
`from ppisp import ppisp_apply` bind to the MI355X module of 3dgrut_amd/ppisp.py unchanged."""
import importlib as _il
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)
_impl = _il.import_module("3dgrut_amd.ppisp")
PPISP, PPISPConfig, ppisp_apply = _impl.PPISP, _impl.PPISPConfig, _impl.ppisp_apply

__all__ = ["PPISP", "PPISPConfig", "ppisp_apply"]
