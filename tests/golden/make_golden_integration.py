#!/usr/bin/env python3
"""INTEGRATION.md section 1 applied to the reference's OWN model files, recorded as data (integration_decoder.json) so that the test that checks
the mirrors against them (tests/test_host_logic.py::test_reference_model_files_import_against_the_mirrors) needs no copy of the reference.

With the sys.modules aliases of INTEGRATION.md section 1 in place this script imports the reference's networks/aoc/aocnet.py and
networks/aoc/decoding_module.py, builds the reference's decoder with the arguments aocnet.py:37-42 passes (configs/resnet101_aocnet.py:
100 + 64, 400, 256, 64, 256) and DynamicPreHead(24, 64), and records:

  * ``imports``: every name the two files bind from an aliased module, and which mirror module it came from;
  * ``calls``: every constructor call the reference's decoder makes of a mirror class (the attribute it lands in, the class, the positional and
    keyword arguments as written -- e.g. the ``attention_dim=`` keyword it passes to conditioning_block) and the parameter shapes it produced;
  * ``state_dict``: name -> shape of the decoder's and of DynamicPreHead's parameters and buffers.

Two names the decoder's constructor reads are undefined in the reference (decoding_module.py:21 ``unc_topk_ratio``, :30 ``self.beta_percentage``):
they are injected (0.3), nothing else is touched.  CPU only: constructors, no forward.

    python tests/golden/make_golden_integration.py <the reference's complete_project/AOCNet directory>
"""
import importlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def main(ref_root):
    sys.dont_write_bytecode = True                       # never write into the reference tree
    sys.path.insert(0, ref_root)
    sys.path.insert(0, REPO)
    import aoc_amd
    aliases = {"networks.layers.matching": aoc_amd.matching, "networks.layers.attention": aoc_amd.attention,
               "networks.aoc.conditioning_layer": aoc_amd.conditioning_layer, "networks.p2t.conditioning_layer": aoc_amd.conditioning_layer,
               "networks.layers.gct": aoc_amd.gct}      # the reference's gct.py imports networks.p2t.center_module, which it does not ship
    sys.modules.update(aliases)
    mirror_of = {id(m): m.__name__.split(".")[-1] for m in aliases.values()}
    dm = importlib.import_module("networks.aoc.decoding_module")
    sys.modules["networks.p2t.decoding_module"] = dm    # aocnet.py:8 names a path the reference does not ship: its own decoder module
    an = importlib.import_module("networks.aoc.aocnet")

    def bound_names(mod):
        """Names the file binds to objects of a mirror module (functions and classes defined there)."""
        out = {}
        for name, obj in vars(mod).items():
            home = sys.modules.get(getattr(obj, "__module__", None) or "")
            if (inspect.isfunction(obj) or inspect.isclass(obj)) and home is not None and id(home) in mirror_of:
                out[name] = mirror_of[id(home)]
            elif inspect.ismodule(obj) and id(obj) in mirror_of:
                out[name] = mirror_of[id(obj)]
        return out

    imports = {"aocnet": bound_names(an), "decoding_module": bound_names(dm)}

    # every constructor call of a mirror class made directly by the reference's decoder constructor (calls nested inside a mirror are the mirror's own)
    classes = {c: mirror_of[id(sys.modules[c.__module__])] for c in {v for v in vars(dm).values() if inspect.isclass(v)}
               if id(sys.modules.get(c.__module__)) in mirror_of}
    calls, depth = [], [0]
    originals = {}
    for cls in classes:
        originals[cls] = cls.__init__

        def init(self, *a, _cls=cls, **k):
            top = depth[0] == 0
            depth[0] += 1
            try:
                originals[_cls](self, *a, **k)
            finally:
                depth[0] -= 1
            if top and type(self) is _cls:
                calls.append(dict(obj=self, module=classes[_cls], cls=_cls.__name__, args=list(a), kwargs=dict(k)))
        cls.__init__ = init
    dm.unc_topk_ratio = 0.3
    dm.CalibrationDecoding.beta_percentage = 0.3
    dec = dm.CalibrationDecoding(in_dim=164, attention_dim=400, embed_dim=256, refine_dim=64, low_level_dim=256)
    for cls, f in originals.items():
        cls.__init__ = f
    where = {id(m): n for n, m in dec.named_modules()}
    shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}
    rec_calls = [dict(attr=where[id(c["obj"])], module=c["module"], cls=c["cls"], args=c["args"], kwargs=c["kwargs"], state_dict=shapes(c["obj"]))
                 for c in calls if id(c["obj"]) in where]
    pre = dm.DynamicPreHead(in_dim=24, embed_dim=64)
    out = dict(imports=imports, calls=rec_calls, state_dict=dict(decoder=shapes(dec), DynamicPreHead=shapes(pre)),
               decoder_class=type(dec).__name__, prehead_is_reference_class=type(pre).__module__ == dm.__name__)
    with open(os.path.join(HERE, "integration_decoder.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("integration_decoder.json:", len(rec_calls), "constructor calls,", len(out["state_dict"]["decoder"]), "decoder tensors")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
