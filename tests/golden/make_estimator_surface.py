"""Build container only: derive, from the reference's OWN files, the surface of its state estimator that the drop-in
quadruped-reactive-walking_amd/Estimator.py has to provide, and write it as tests/golden/estimator_surface.json (names and
arities only -- no source text travels).

  python tests/golden/make_estimator_surface.py [/root/reference]

What is walked, with `ast`:
  scripts/Estimator.py    class Estimator: per method the (min, max) number of positional arguments a caller may pass (self
                          excluded), the constructor's argument names and the attributes the class assigns on self;
  scripts/Controller.py   every attribute chain rooted at self.estimator: the attributes read and the methods called with their
                          positional-argument counts.
tests/test_estimator_cpu.py asserts that the drop-in provides every entry (logging and plotting are listed there as not provided)."""
import ast
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "estimator_surface.json")
ROOT_CHAIN = "self.estimator"


def chain(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if isinstance(node, ast.Name):
        parts.append(node.id)
        return ".".join(reversed(parts))
    return None


def walk_definition(path, class_name="Estimator"):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == class_name:
            methods, attrs, ctor = {}, set(), []
            for f in node.body:
                if not isinstance(f, ast.FunctionDef):
                    continue
                a = f.args
                npos = len(a.args) - 1
                methods[f.name] = [npos - len(a.defaults), npos]
                if f.name == "__init__":
                    ctor = [x.arg for x in a.args[1:]]
                for n in ast.walk(f):
                    if (isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Store) and isinstance(n.value, ast.Name)
                            and n.value.id == "self"):
                        attrs.add(n.attr)
            return {"methods": dict(sorted(methods.items())), "attributes": sorted(attrs), "constructor": ctor}
    raise SystemExit("no class %s in %s" % (class_name, path))


def walk_uses(path):
    tree = ast.parse(open(path).read())
    reads, calls = set(), {}
    called = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Call):
            d = chain(node.func)
            if d and d.startswith(ROOT_CHAIN + "."):
                called.add(id(node.func))
                rest = d[len(ROOT_CHAIN) + 1:].split(".")
                if len(rest) == 1:
                    calls.setdefault(rest[0], set()).add(len(node.args))
                else:
                    reads.add(rest[0])
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and id(node) not in called:
            d = chain(node)
            if d and d.startswith(ROOT_CHAIN + "."):
                reads.add(d[len(ROOT_CHAIN) + 1:].split(".")[0])
    reads -= set(calls)
    return {"reads": sorted(reads), "calls": {k: sorted(v) for k, v in sorted(calls.items())}}


def surface(ref):
    return {"generated_by": "tests/golden/make_estimator_surface.py", "reference": "paLeziart/quadruped-reactive-walking",
            "definition": {"file": "scripts/Estimator.py", "class": walk_definition(os.path.join(ref, "scripts", "Estimator.py"))},
            "uses": {"scripts/Controller.py": walk_uses(os.path.join(ref, "scripts", "Controller.py"))}}


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    s = surface(ref)
    json.dump(s, open(OUT, "w"), indent=1, sort_keys=True)
    print("wrote %s: %d methods, %d attributes, %d reads / %d calls in Controller.py"
          % (OUT, len(s["definition"]["class"]["methods"]), len(s["definition"]["class"]["attributes"]),
             len(s["uses"]["scripts/Controller.py"]["reads"]), len(s["uses"]["scripts/Controller.py"]["calls"])))
