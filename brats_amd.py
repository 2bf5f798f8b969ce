"""Importable alias of the hot-path package.

The package directory carries the name the build contract prescribes
(``automated-brain-mri-...-assistance_amd``), which is not a Python identifier; this shim
loads it once and aliases it (and its submodules) as ``brats_amd``.

``python -m brats_amd.X`` for a submodule X that the package itself imports (``evaluate``): runpy
asks the loader of whatever ``sys.modules["brats_amd.X"]`` holds for the code of "brats_amd.X",
which the loader of the long-named module refuses.  That one alias is therefore left out while X
is the ``-m`` target, so that runpy finds X by path under the alias, as it does for the submodules
that are imported on demand.
"""
import importlib
import sys

_LONG = "automated-brain-mri-analysis-and-report-generation-with-retrieval-augmented-clinical-assistance_amd"
_argv = list(getattr(sys, "orig_argv", []))
_target = _argv[_argv.index("-m") + 1] if sys.argv[:1] == ["-m"] and "-m" in _argv[:-1] else None
_pkg = importlib.import_module(_LONG)
for _k, _v in list(sys.modules.items()):
    if (_k == _LONG or _k.startswith(_LONG + ".")) and "brats_amd" + _k[len(_LONG):] != _target:
        sys.modules["brats_amd" + _k[len(_LONG):]] = _v
sys.modules[__name__] = _pkg
