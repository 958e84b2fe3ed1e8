"""Dumps ``default_tune_range`` of every recommender class of the reference to ``tests/golden/tune_ranges.json``
(run in the build container, where ``/root/reference`` exists: ``python tests/golden/make_tune_ranges.py``).
The output is data - per class, the list of ``{name, kind, low, high, step, choices}`` - that
``tests/test_tune_surface.py`` compares the classes of ``irspack_amd.recommenders`` with; the reference's text is not
kept.  Like ``make_api_surface.py`` it reads the files with ``ast`` and imports nothing of the reference.

Sources: src/irspack/optimization/parameter_range.py (the two shared kNN lists) and the class bodies in
src/irspack/recommenders/{p3,rp3,knn,user_knn,slim,dense_slim,edlae,truncsvd,nmf,bpr,multvae,ials,toppop}.py
"""
import ast
import json
import os
import sys

REF = os.environ.get("IRSPACK_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

SHARED = "src/irspack/optimization/parameter_range.py"
MODULES = ["p3", "rp3", "knn", "user_knn", "slim", "dense_slim", "edlae", "truncsvd", "nmf", "bpr", "multvae",
           "ials", "toppop"]
# constructor arguments of the range classes, in order
ARGS = {
    "UniformFloatRange": ("uniform_float", ["name", "low", "high"]),
    "LogUniformFloatRange": ("log_uniform_float", ["name", "low", "high"]),
    "UniformIntegerRange": ("uniform_int", ["name", "low", "high", "step"]),
    "LogUniformIntegerRange": ("log_uniform_int", ["name", "low", "high"]),
    "CategoricalRange": ("categorical", ["name", "choices"]),
}


def one_range(call: ast.Call) -> dict:
    kind, names = ARGS[call.func.id]
    given = {name: ast.literal_eval(arg) for name, arg in zip(names, call.args)}
    given.update({kw.arg: ast.literal_eval(kw.value) for kw in call.keywords})
    entry = dict(name=given["name"], kind=kind, low=given.get("low"), high=given.get("high"), step=None,
                 choices=given.get("choices"))
    if kind == "uniform_int":
        entry["step"] = given.get("step", 1)
    return entry


def ranges(node: ast.AST, shared: dict) -> list:
    """the list an expression of range constructors, shared lists, ``.copy()`` and ``+`` stands for"""
    if isinstance(node, ast.List):
        return [one_range(item) for item in node.elts]
    if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Add):
        return ranges(node.left, shared) + ranges(node.right, shared)
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "copy":
        return ranges(node.func.value, shared)
    if isinstance(node, ast.Name):
        return list(shared[node.id])
    raise ValueError(f"cannot read {ast.dump(node)}")


def assigned(body: list, shared: dict) -> dict:
    """``{target: ranges}`` of the assignments in ``body`` whose target is named ``default_tune_range*``"""
    out = {}
    for node in body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
            target, value = node.targets[0].id, node.value
        elif isinstance(node, ast.AnnAssign) and isinstance(node.target, ast.Name) and node.value is not None:
            target, value = node.target.id, node.value
        else:
            continue
        if target.startswith("default_tune_range"):
            out[target] = ranges(value, dict(shared, **out))
    return out


def parse(rel: str) -> ast.Module:
    path = os.path.join(REF, rel)
    if not os.path.exists(path):
        sys.exit(f"{path} not found: this script runs where the reference checkout is")
    return ast.parse(open(path).read())


def main() -> None:
    shared = assigned(parse(SHARED).body, {})
    result = {}
    for module in MODULES:
        for node in parse(f"src/irspack/recommenders/{module}.py").body:
            if isinstance(node, ast.ClassDef):
                found = assigned(node.body, shared)
                if "default_tune_range" in found:
                    result[node.name] = found["default_tune_range"]
    with open(os.path.join(HERE, "tune_ranges.json"), "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
