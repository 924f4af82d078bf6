"""Golden record of the reference's argument parser (TPT/params.py:13-98): every option it declares, with its option strings and the
default it parses to, so that the mirror in rlcf_amd.params is checked without the reference at hand.

    python tests/golden/make_params_golden.py /path/to/TPT/params.py

params_ref.json   {"argv": [...], "actions": [{"dest", "option_strings", "default"}, ...]}
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ARGV = ["/data", "--output", "/tmp/rlcf_params_test"]      # the positional data root and the output folder the parser requires


def main():
    captured = {}
    real_parse = argparse.ArgumentParser.parse_args

    def fake_parse(self, args=None, namespace=None):
        captured["parser"] = self
        return real_parse(self, ARGV, namespace)
    spec = importlib.util.spec_from_file_location("ref_params", sys.argv[1])
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    argparse.ArgumentParser.parse_args = fake_parse
    try:
        spec.loader.exec_module(mod)
        mod.save_hp_to_json = lambda *a, **k: None
        ns = mod.get_args()
    finally:
        argparse.ArgumentParser.parse_args = real_parse
    actions = [{"dest": a.dest, "option_strings": list(a.option_strings), "default": getattr(ns, a.dest)}
               for a in captured["parser"]._actions if a.dest != "help"]
    with open(os.path.join(HERE, "params_ref.json"), "w") as f:
        json.dump({"argv": ARGV, "actions": actions}, f, indent=1)
        f.write("\n")
    print(f"{len(actions)} options")


if __name__ == "__main__":
    main()
