"""``python scripts/code_lines.py FILE...``: the code lines of Python files — lines that are not blank, not comments
and not docstrings — per file and in total (the size measure of refactors)."""
import ast
import sys
import tokenize

SKIP = (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER)


def code_lines(path):
    with open(path) as fh:
        src = fh.read()
    doc = set()
    for n in ast.walk(ast.parse(src)):
        if isinstance(n, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and ast.get_docstring(n):
            doc.update(range(n.body[0].lineno, n.body[0].end_lineno + 1))
    with open(path) as fh:
        code = {line for t in tokenize.generate_tokens(fh.readline) if t.type not in SKIP
                for line in range(t.start[0], t.end[0] + 1)}
    return len(code - doc)


if __name__ == '__main__':
    counts = [(p, code_lines(p)) for p in sys.argv[1:]]
    for p, n in counts:
        print(f'{n:6d} {p}')
    print(f'{sum(n for _, n in counts):6d} total')
