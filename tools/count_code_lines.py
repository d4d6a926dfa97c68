"""Code lines of Python files: the lines that carry a token other than a comment or a docstring (tokens by ``tokenize``, docstring
lines by ``ast``), per file and in total -- the figure ``profiles/helpers_split.md`` compares.
python tools/count_code_lines.py dae_rnn_news_recommendation_amd/helpers/*.py"""
import ast
import io
import sys
import tokenize


def code_lines(path):
    src = open(path).read()
    doc = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body:
            e = node.body[0]
            if isinstance(e, ast.Expr) and isinstance(e.value, ast.Constant) and isinstance(e.value.value, str):
                doc.update(range(e.lineno, e.end_lineno + 1))
    skip = {tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENCODING, tokenize.ENDMARKER}
    lines = set()
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type in skip:
            continue
        for ln in range(tok.start[0], tok.end[0] + 1):
            if ln not in doc:
                lines.add(ln)
    return len(lines)


total = 0
for p in sys.argv[1:]:
    n = code_lines(p)
    total += n
    print(f"{n:6d}  {p}")
print(f"{total:6d}  total")
