"""`ppisp.report` of the shadowed package: `threedgrut/trainer.py:988` (`from ppisp.report import export_ppisp_report`)."""
import importlib as _il

export_ppisp_report = _il.import_module("3dgrut_amd.ppisp").export_ppisp_report

__all__ = ["export_ppisp_report"]
