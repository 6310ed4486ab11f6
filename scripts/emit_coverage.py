"""``python scripts/emit_coverage.py``: the statements of the stencil emitter (every ``.py`` file of
``backends/hip_emitter`` and ``backends/hip_band`` — each the package, or the one module) that neither pinned generator
executes, per function: ``rows()`` of ``tests/golden/make_emit_golden.py`` and ``periodic_rows()`` of
``tests/test_periodic_march.py`` run under a ``sys.settrace`` line collector (no coverage package needed). ``raise``
statements are listed apart: the generators are complete when nothing else is left, and the exit status says so.
Then the size listing: the total lines of each file and the ten longest top-level functions (``def`` line to last
line, nested functions included)."""
import ast
import glob
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKENDS = os.path.join(ROOT, 'pystencils_autodiff_amd', 'backends')
FILES = [path for name in ('hip_emitter', 'hip_band')
         for path in sorted(glob.glob(os.path.join(BACKENDS, name + '.py')) +
                            glob.glob(os.path.join(BACKENDS, name, '*.py')))]


def parse(path):
    with open(path) as fh:
        text = fh.read()
    return ast.parse(text), text.count('\n')


def statements(tree):
    """``[(function, first line, last own line, is_raise)]`` of every statement inside a function: a compound
    statement counts with its header lines only, docstrings and ``global`` / ``nonlocal`` do not count."""
    out = []

    def visit(node, func):
        for child in ast.iter_child_nodes(node):
            name = func
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                name = f'{func}.{child.name}' if func else child.name
            if isinstance(child, ast.stmt) and func and not isinstance(child, (ast.Global, ast.Nonlocal)) and \
                    not (isinstance(child, ast.Expr) and isinstance(child.value, ast.Constant)):
                inner = [s.lineno for s in ast.walk(child) if isinstance(s, ast.stmt) and s is not child]
                first = child.lineno
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) and child.decorator_list:
                    first = child.decorator_list[0].lineno
                out.append((func, first, min(inner) - 1 if inner else child.end_lineno, isinstance(child, ast.Raise)))
            visit(child, name)
    visit(tree, '')
    return out


def top_level_functions(tree):
    """``[(lines, name)]`` of the module's own functions: ``def`` line to last line, nested functions included."""
    return [(n.end_lineno - n.lineno + 1, n.name) for n in tree.body
            if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]


def collect(files, run):
    hit = {os.path.realpath(f): set() for f in files}
    known = {}                      # file name as the code object has it -> its line set, or None

    def local(frame, event, arg):
        if event == 'line':
            known[frame.f_code.co_filename].add(frame.f_lineno)
        return local

    def tracer(frame, event, arg):
        name = frame.f_code.co_filename
        if name not in known:
            known[name] = hit.get(os.path.realpath(name))
        if known[name] is None:
            return None
        known[name].add(frame.f_lineno)
        return local
    sys.settrace(tracer)
    try:
        run()
    finally:
        sys.settrace(None)
    return hit


def load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    gen = load('make_emit_golden', 'tests', 'golden', 'make_emit_golden.py')      # (puts ROOT on sys.path)
    periodic = load('test_periodic_march', 'tests', 'test_periodic_march.py')

    def run():
        gen.rows()
        periodic.periodic_rows()
    hit = collect(FILES, run)
    missed = 0
    sizes, functions = [], []
    for path in FILES:
        rel = os.path.relpath(path, ROOT)
        tree, nlines = parse(path)
        sizes.append((nlines, rel))
        functions += [(n, f'{rel}: {name}') for n, name in top_level_functions(tree)]
        stmts = statements(tree)
        lines = hit[os.path.realpath(path)]
        left = [(fn, a, b, r) for fn, a, b, r in stmts if not lines.intersection(range(a, b + 1))]
        other = [s for s in left if not s[3]]
        missed += len(other)
        print(f'{rel}: {len(stmts) - len(left)} of {len(stmts)} statements executed, '
              f'{len(left) - len(other)} raise and {len(other)} other statements never')
        for kind, sel in (('raise', [s for s in left if s[3]]), ('NEVER', other)):
            by_fn = {}
            for fn, a, b, _ in sel:
                by_fn.setdefault(fn, []).append(str(a) if a == b else f'{a}-{b}')
            for fn, spans in by_fn.items():
                print(f'  {kind} {fn}: {" ".join(spans)}')
    print('lines per file:')
    for n, rel in sizes:
        print(f'  {n:5d} {rel}')
    print('longest top-level functions:')
    for n, name in sorted(functions, key=lambda t: -t[0])[:10]:
        print(f'  {n:5d} {name}')
    return 1 if missed else 0


if __name__ == '__main__':
    sys.exit(main())
