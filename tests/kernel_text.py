"""Cuts named definitions out of a .hip / .inc / .h file, so that a CPU test program can compile the SHIPPED text of a kernel, a device
helper, a launcher, a struct or a constant behind stand-ins for the HIP names (tests/kernel_emu.h), without touching the library's
sources or build.

    extract(path, "gf2_xor2d_kernel")          -> the text of that one definition, a preceding `template <...>` included
    extract_all(path, ["xor4", "gf2k_xor2d"])  -> the definitions joined, in the order asked for

A definition of NAME is one of
    NAME ( ... ) {  ... }          a function (a kernel, a __device__ helper, an extern "C" launcher)
    struct NAME { ... };           a struct
    NAME = ... ;  /  NAME[..] = ... ;   a variable or constant
and begins behind the previous `;`, `{` or `}` (comments, blank lines and preprocessor lines skipped).  Calls, declarations and uses
inside other bodies do not match these shapes.  Braces, parentheses and the words searched for are looked at only outside comments,
string and character literals.  KeyError if the name has no definition, ValueError if it has more than one.
"""
import re


def mask(text):
    """text with every comment and the inside of every string / character literal turned into blanks: offsets and newlines kept"""
    out = list(text)
    i, n = 0, len(text)

    def blank(a, b):
        for k in range(a, b):
            if out[k] != "\n":
                out[k] = " "

    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            blank(i, j)
            i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            blank(i, j)
            i = j
        elif c == '"' or (c == "'" and not (i > 0 and text[i - 1].isalnum())):  # 1'000 is a digit separator, not a literal
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            blank(i + 1, min(j, n))
            i = j + 1
        else:
            i += 1
    return "".join(out)


def _match(m, i, open_, close):
    """index just behind the bracket that closes the one at m[i]"""
    depth = 0
    for j in range(i, len(m)):
        if m[j] == open_:
            depth += 1
        elif m[j] == close:
            depth -= 1
            if depth == 0:
                return j + 1
    raise ValueError("unbalanced %s at offset %d" % (open_, i))


def _statement_end(m, i):
    """index just behind the `;` that ends the statement running through m[i], braces and parentheses skipped"""
    while i < len(m):
        if m[i] == "{":
            i = _match(m, i, "{", "}")
        elif m[i] == "(":
            i = _match(m, i, "(", ")")
        elif m[i] == ";":
            return i + 1
        else:
            i += 1
    raise ValueError("statement without end")


def _start(m, at):
    """where the definition that names itself at m[at] begins"""
    i = at
    while i > 0 and m[i - 1] not in ";{}":
        i -= 1
    while True:  # forward over blank lines and preprocessor lines
        while i < at and m[i].isspace():
            i += 1
        if m[i] == "#":
            i = m.index("\n", i)
        else:
            return i


def _definitions(text, name):
    m = mask(text)
    found = []
    for hit in re.finditer(r"(?<![\w.>])%s\b\s*" % re.escape(name), m):
        j = hit.end()
        if j >= len(m):
            continue
        end = None
        if m[j] == "(":
            k = _match(m, j, "(", ")")
            rest = re.match(r"\s*(const\s*|noexcept\s*)*\{", m[k:])
            if rest:
                end = _match(m, k + rest.end() - 1, "{", "}")
        elif m[j] == "{" and re.search(r"\b(struct|class|union)\s+$", m[: hit.start()]):
            end = _statement_end(m, j)
        elif m[j] == "[" or (m[j] == "=" and m[j + 1] != "="):
            start = _start(m, hit.start())
            # a definition's statement begins with a type, not with the name: `x = 1;` inside a body is an assignment
            if start < hit.start() and not re.search(r"[(=,?:]", m[start:hit.start()].replace("::", "")):
                end = _statement_end(m, j)
        if end is not None:
            found.append((_start(m, hit.start()), end))
    return found


def extract(path, name):
    with open(path) as f:
        text = f.read()
    found = _definitions(text, name)
    if not found:
        raise KeyError("%s: no definition of %s" % (path, name))
    if len(found) > 1:
        raise ValueError("%s: %d definitions of %s" % (path, len(found), name))
    a, b = found[0]
    return text[a:b] + "\n"


def extract_all(path, names):
    return "\n".join(extract(path, n) for n in names)


def global_kernels(path):
    """names of the __global__ definitions of a file, in order"""
    with open(path) as f:
        m = mask(f.read())
    names = []
    for hit in re.finditer(r"\b__global__\b", m):
        k = hit.end()
        while True:  # the first `name (` behind __global__ that is not __launch_bounds__ is the kernel
            w = re.compile(r"\s*(\w+)\s*").match(m, k)
            if not w:
                raise ValueError("%s: __global__ without a name at offset %d" % (path, hit.start()))
            k = w.end()
            if m[k] == "(":
                if w.group(1) == "__launch_bounds__":
                    k = _match(m, k, "(", ")")
                    continue
                names.append(w.group(1))
                break
    return names
