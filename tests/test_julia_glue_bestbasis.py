"""Lint of the best-basis Julia glue (wavelets.jl_amd/julia/WaveletsMI355X_bestbasis.jl) -- CPU only, the same rules as
tests/test_julia_glue.py applies to WaveletsMI355X.jl:
  * every `ccall` matches _lib.SIGNATURES (name, return type, arity, each argument type), and the glue binds both new entry points;
  * every pointer(...) handed to C is kept alive by GC.@preserve;
  * every method it adds is element-wise `<:` a reference method of the same name and arity, here the methods of
    src/Threshold/entropy.jl in tests/golden/reference_bestbasis_signatures.json (tools/gen_seam_signatures.py --out ... --names
    bestbasistree,coefentropy --files src/Threshold/entropy.jl), so Julia's dispatch picks it without ambiguity;
  * the module includes the file.
"""
import json
import os
import re

import test_julia_glue as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "wavelets.jl_amd", "julia")
GLUE = os.path.join(JL, "WaveletsMI355X_bestbasis.jl")
SEAM = os.path.join(ROOT, "tests", "golden", "reference_bestbasis_signatures.json")


def _ccalls(path):
    src = re.sub(r"#[^\n]*", "", open(path).read())
    calls = []
    for m in re.finditer(r"ccall\(", src):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            j += 1
        parts = G._split_top(src[m.end():j - 1])
        ls = src.rfind("\n", 0, m.start()) + 1
        calls.append({"sym": re.match(r"\(:(\w+),\s*LIB\)", parts[0]).group(1), "ret": parts[1],
                      "types": G._split_top(parts[2].strip()[1:-1]), "args": parts[3:], "line": src.count("\n", 0, m.start()) + 1,
                      "prefix": src[ls:m.start()]})
    return calls


def test_module_includes_the_file():
    assert re.search(r'^include\("WaveletsMI355X_bestbasis\.jl"\)$', open(os.path.join(JL, "WaveletsMI355X.jl")).read(), re.M)


def test_every_ccall_matches_the_abi():
    from wavelets_jl_amd import _lib
    calls = _ccalls(GLUE)
    assert {c["sym"] for c in calls} == {"wl_coefentropy", "wl_bestbasistree_filter"}
    for c in calls:
        restype, argtypes = _lib.SIGNATURES[c["sym"]]
        assert G.JL2C[c["ret"]] is restype, (c["sym"], c["line"])
        assert len(c["types"]) == len(argtypes) == len(c["args"]), (c["sym"], c["line"], len(c["types"]), len(argtypes), len(c["args"]))
        for k, (jt, ct) in enumerate(zip(c["types"], argtypes)):
            assert G.JL2C[jt] is ct, "%s (line %d) argument %d: Julia %s, ABI %s" % (c["sym"], c["line"], k + 1, jt, ct)


def test_device_pointers_are_gc_preserved():
    for c in _ccalls(GLUE):
        names = [m.group(1) for a in c["args"] for m in re.finditer(r"pointer\((\w+)\)", a)]
        assert names, c["sym"]
        m = re.search(r"GC\.@preserve\s+([\w\s]+?)\s+check\($", c["prefix"].rstrip())
        assert m, "%s (line %d): pointer(...) passed to C outside GC.@preserve" % (c["sym"], c["line"])
        assert set(names) <= set(m.group(1).split()), (c["sym"], c["line"])


def test_every_method_is_a_subtype_of_a_reference_method():
    seam = json.load(open(SEAM))
    assert set(seam["methods"]) == {"bestbasistree", "coefentropy"}
    ms = G._glue_methods(open(GLUE).read())
    arities = sorted((g["name"], len(g["params"])) for g in ms)
    # bestbasistree: the tree form (3, 4 arguments) and the L form (2, 3, 4); coefentropy with and without nrm
    assert arities == sorted([("bestbasistree", 3), ("bestbasistree", 4), ("bestbasistree", 2), ("bestbasistree", 3),
                              ("bestbasistree", 4), ("coefentropy", 3), ("coefentropy", 2)]), arities
    for g in ms:
        at = [r["at"] for r in seam["methods"][g["name"]] if G._method_sub(g, r, seam["aliases"])]
        assert at, "glue method %s(%s) [line %d] is not element-wise <: any reference method of that name and arity" % (
            g["name"], ", ".join(g["params"]), g["line"])


def test_lint_is_not_vacuous():
    """signatures that are not subtypes of entropy.jl's methods are rejected: any-rank arrays against AbstractVector, a host
    Vector{Bool} tree against BitVector, a Float32-only nrm slot against the shared element type"""
    seam = json.load(open(SEAM))
    bad = '''
function Threshold.bestbasistree(y::ROCArray{T}, wt::OrthoFilter, tree::BitVector) where {T<:Union{Float32,Float64}}
end
function Threshold.bestbasistree(y::ROCVector{T}, wt::OrthoFilter, tree::Vector{Bool}) where {T<:Union{Float32,Float64}}
end
function Threshold.coefentropy(x::ROCArray{T}, et::Entropy, nrm::Float32) where {T<:Union{Float32,Float64,Int}}
end
'''
    ms = G._glue_methods(bad)
    assert len(ms) == 3
    for g in ms:
        assert not [r for r in seam["methods"][g["name"]] if G._method_sub(g, r, seam["aliases"])], g
