"""The one reader of include/eigentraj.h for the tests: its text without comments, the function prototypes, the integer
``#define``s and the field names of its structs."""
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "include", "eigentraj.h")


@functools.lru_cache(maxsize=None)
def text():
    """The header with every comment removed."""
    with open(PATH) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


@functools.lru_cache(maxsize=None)
def functions():
    """{name: (return type, [argument types])} in the header's order, as C spellings without parameter names and with
    single spaces ("const float *", "int64_t", "et_kmeans_state *const *")."""
    out = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+[\s*]+)(et_\w+)\s*\(([^)]*)\)\s*;", text(), flags=re.M):
        params = [] if params.strip() == "void" else [re.sub(r"\w+$", "", p.strip()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [" ".join(p.split()) for p in params])
    return out


@functools.lru_cache(maxsize=None)
def defines():
    """{name: int} of the ``#define``s whose value is an integer literal."""
    return {name: int(value) for name, value in re.findall(r"^#define\s+(\w+)\s+(-?\d+)\s*$", text(), flags=re.M)}


def struct_fields(name):
    """Field names of ``typedef struct name {...} name;`` in declaration order."""
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", text(), re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"\[[^\]]*\]", "", decl).strip()
        if decl:
            names += [n.strip(" *") for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    return names
