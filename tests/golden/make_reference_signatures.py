"""Derive the metadata of the reference package that tests/test_julia_binding.py checks the binding and the recipe against (names,
types, UUIDs, bounds and `file:line` only — metadata, not source), from a checkout of impICNF/ContinuousNormalizingFlows.jl v0.31.0:

  reference_signatures.json            argument-type table of the reference methods the HIP binding specialises
  reference_constructor_keywords.json  keyword names of the `ICNF(; ...)` constructor
  reference_types.json                 the struct names src/core/types.jl declares
  reference_project.json               [deps] UUIDs and [compat] bounds of the reference's Project.toml

Run from the repo root:  python tests/golden/make_reference_signatures.py REFERENCE_DIR            (rewrite the fixtures)
                         python tests/golden/make_reference_signatures.py --check REFERENCE_DIR    (exit 1 if any is stale)
REFERENCE_DIR may also be given as the environment variable CNF_REFERENCE."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from jl_signatures import methods  # noqa: E402

REF = os.environ.get("CNF_REFERENCE")
NAMES = ("augmented_f", "base_sol", "inference_sol", "generate_sol", "make_ode_func", "loss", "inference_prob", "rrule",
         # called by julia/make_reference_golden.jl (arity / argument-kind check in tests/test_julia_binding.py)
         "inference", "add_conditions_nn")
FILES = ("src/core/icnf.jl", "src/core/base_icnf.jl", "src/core/utils.jl")


def derive():
    table = []
    for f in FILES:
        text = open(os.path.join(REF, f)).read()
        for name, types, line in methods(text, NAMES):
            table.append({"function": name, "args": types, "where": f"{f}:{line}"})
    return table


def constructor_keywords():
    """Keyword names of the reference's `ICNF(; ...)` constructor (src/core/icnf.jl:53-103) - names only."""
    text = open(os.path.join(REF, "src/core/icnf.jl")).read()
    start = text.index("function ICNF(;")
    depth, i = 0, text.index("(", start)
    j = i
    while True:
        c = text[j]
        depth += c == "("
        depth -= c == ")"
        if depth == 0:
            break
        j += 1
    from jl_signatures import split_top
    kws = []
    for a in split_top(text[i + 2:j].replace("\n", " ")):
        m = re.match(r"\s*([^\s:=]+)\s*(::|=)", a)
        if m:
            kws.append(m.group(1))
    return kws


def type_names():
    """Names of the structs src/core/types.jl declares (the compute modes and modes) - names only."""
    return re.findall(r"\bstruct\s+(\w+)", open(os.path.join(REF, "src/core/types.jl")).read())


def project():
    """{deps: name -> UUID, compat: name -> bound} of the reference's Project.toml."""
    import tomli
    p = tomli.load(open(os.path.join(REF, "Project.toml"), "rb"))
    return {"deps": p["deps"], "compat": p["compat"]}


FIXTURES = {"reference_signatures.json": derive, "reference_constructor_keywords.json": constructor_keywords,
            "reference_types.json": type_names, "reference_project.json": project}


if __name__ == "__main__":
    args = sys.argv[1:]
    check = "--check" in args
    args = [a for a in args if a != "--check"]
    REF = args[0] if args else REF
    if not REF or not os.path.isdir(os.path.join(REF, "src", "core")):
        sys.exit(f"usage: {sys.argv[0]} [--check] REFERENCE_DIR (a checkout of ContinuousNormalizingFlows.jl; or set CNF_REFERENCE)")
    stale = []
    for fn, make in FIXTURES.items():
        path = os.path.join(HERE, fn)
        if check:
            if make() != json.load(open(path)):
                stale.append(fn)
        else:
            json.dump(make(), open(path, "w"), indent=0)
    if stale:
        sys.exit("stale: " + ", ".join(stale))
    print("fixtures " + ("current" if check else "written") + f": {', '.join(FIXTURES)}")
