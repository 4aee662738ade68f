"""The layout of the tests' support code: shared checks live in plain helper modules (icp_checks.py, the *_ref.py restatements), so
that an edit to one feature's test module cannot change what another module asserts."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _imports(tree):
    """Every module name an import statement names, at module level or inside a function."""
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield node.lineno, a.name
        elif isinstance(node, ast.ImportFrom):
            yield node.lineno, node.module or ""


def test_no_test_module_imports_a_test_module():
    bad = []
    paths = sorted(glob.glob(os.path.join(HERE, "test_*.py")))
    assert len(paths) > 30, paths
    for path in paths:
        tree = ast.parse(open(path).read(), path)
        bad += ["%s:%d imports %s" % (os.path.basename(path), line, name) for line, name in _imports(tree)
                if name.split(".")[-1].startswith("test_")]
    assert not bad, bad


def test_the_support_module_holds_no_test():
    tree = ast.parse(open(os.path.join(HERE, "icp_checks.py")).read())
    names = [n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    names += [t.id for n in ast.walk(tree) if isinstance(n, ast.Assign) for t in n.targets if isinstance(t, ast.Name)]
    names += [(a.asname or a.name) for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for a in n.names]
    assert len(names) > 50 and not [n for n in names if n.startswith("test_")], names
