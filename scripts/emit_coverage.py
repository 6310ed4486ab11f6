"""``python scripts/emit_coverage.py``: the statements of the stencil emitter (``backends/hip_emitter.py`` and
``backends/hip_band.py``) that ``tests/golden/make_emit_golden.py`` never executes, per function (a
``sys.settrace`` line collector: no coverage package needed). ``raise`` statements are listed apart: the generator is
complete when nothing else is left, and the exit status says so."""
import ast
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKENDS = os.path.join(ROOT, 'pystencils_autodiff_amd', 'backends')
FILES = [os.path.join(BACKENDS, 'hip_emitter.py'), os.path.join(BACKENDS, 'hip_band.py')]


def statements(path):
    """``[(function, first line, last own line, is_raise)]`` of every statement inside a function: a compound
    statement counts with its header lines only, docstrings and ``global`` / ``nonlocal`` do not count."""
    with open(path) as fh:
        tree = ast.parse(fh.read())
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


def main():
    spec = importlib.util.spec_from_file_location('make_emit_golden',
                                                  os.path.join(ROOT, 'tests', 'golden', 'make_emit_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    hit = collect(FILES, gen.rows)
    missed = 0
    for path in FILES:
        stmts = statements(path)
        lines = hit[os.path.realpath(path)]
        left = [(fn, a, b, r) for fn, a, b, r in stmts if not lines.intersection(range(a, b + 1))]
        other = [s for s in left if not s[3]]
        missed += len(other)
        print(f'{os.path.relpath(path, ROOT)}: {len(stmts) - len(left)} of {len(stmts)} statements executed, '
              f'{len(left) - len(other)} raise and {len(other)} other statements never')
        for kind, sel in (('raise', [s for s in left if s[3]]), ('NEVER', other)):
            by_fn = {}
            for fn, a, b, _ in sel:
                by_fn.setdefault(fn, []).append(str(a) if a == b else f'{a}-{b}')
            for fn, spans in by_fn.items():
                print(f'  {kind} {fn}: {" ".join(spans)}')
    return 1 if missed else 0


if __name__ == '__main__':
    sys.exit(main())
