"""Shadow of the CUDA-only package `tinycudann` (the reference's model.feature_type: nht): with `<repo>/shims` on PYTHONPATH,
`threedgrut/model/feature_decoder.py:16` (`import tinycudann as tcnn`) binds to the MI355X decoder network of 3dgrut_amd/tcnn.py
unchanged."""
import importlib as _il
import os as _os
import sys as _sys

_root = _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
if _root not in _sys.path:
    _sys.path.insert(0, _root)
_impl = _il.import_module("3dgrut_amd.tcnn")
NetworkWithInputEncoding = _impl.NetworkWithInputEncoding

__all__ = ["NetworkWithInputEncoding"]
