"""Freezes the public surface of ``dae_rnn_news_recommendation_amd.helpers`` into ``helpers_surface.json``: the public names and
``str(inspect.signature(...))`` of every function, class and public method.  ``tests/test_helpers_surface_cpu.py`` holds the
package to it.  The committed file was taken from the single-module ``helpers.py`` the package replaced; run this again only to
ADD names (python tests/golden/make_helpers_surface.py)."""
import inspect
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def surface(module):
    names, sigs = [], {}
    for n in sorted(vars(module)):
        o = getattr(module, n)
        if n.startswith("_") or isinstance(o, types.ModuleType) or n == "annotations":
            continue
        names.append(n)
        if inspect.isfunction(o):
            sigs[n] = str(inspect.signature(o))
        elif inspect.isclass(o):
            sigs[n] = str(inspect.signature(o))
            for m, f in sorted(vars(o).items()):
                if m.startswith("_") and m != "__init__":
                    continue
                if isinstance(f, (classmethod, staticmethod)):
                    f = f.__func__
                if inspect.isfunction(f):
                    sigs[f"{n}.{m}"] = str(inspect.signature(f))
    return {"names": names, "signatures": sigs}


if __name__ == "__main__":
    from dae_rnn_news_recommendation_amd import helpers
    with open(os.path.join(HERE, "helpers_surface.json"), "w") as fh:
        json.dump(surface(helpers), fh, indent=1, sort_keys=True)
