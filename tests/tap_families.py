"""Sparse and one-sided radius-1 tap tables for the stencil schedules, with plain float64 references.

The schedules' printers branch on the tap table (which planes carry taps, which side of the centre a field is read on,
whether there are x neighbours at all); the workloads exercise them with full boxes and symmetric stars only. The
families here are the ordinary stencils in between: upwind differences, boxes without corners, a 2-D operator on a
3-D field, the adjoint of a one-sided difference.

``plain_forward`` / ``plain_adjoint`` state the operation and its transpose directly on padded or rolled arrays:

    forward   out[x]   = Σ w · u[x + o]
    adjoint   diffu[x] = Σ w · diffout[x − o]

They use neither the autodiff derivation, nor ``oracle.evaluate``, nor any kernel of the project, so a test against
them checks the derived backward assignments as well as the kernels that run them."""
import numpy as np
import sympy as sp

# every weight of the 3-D families comes from this table: 27 literals of magnitude 0.1 .. 1, mixed signs, no two equal
BOX = {
    (-1, -1, -1): 0.31, (-1, -1, 0): -0.47, (-1, -1, 1): 0.12,
    (-1, 0, -1): -0.83, (-1, 0, 0): 0.59, (-1, 0, 1): 0.26,
    (-1, 1, -1): -0.15, (-1, 1, 0): 0.72, (-1, 1, 1): -0.38,
    (0, -1, -1): 0.44, (0, -1, 0): -0.91, (0, -1, 1): 0.17,
    (0, 0, -1): 0.63, (0, 0, 0): -0.55, (0, 0, 1): 0.29,
    (0, 1, -1): -0.22, (0, 1, 0): 0.86, (0, 1, 1): -0.68,
    (1, -1, -1): -0.19, (1, -1, 0): 0.77, (1, -1, 1): -0.34,
    (1, 0, -1): 0.52, (1, 0, 0): -0.11, (1, 0, 1): 0.95,
    (1, 1, -1): 0.41, (1, 1, 0): -0.65, (1, 1, 1): 0.23,
}
BOX2 = {
    (-1, -1): 0.37, (-1, 0): -0.58, (-1, 1): 0.14,
    (0, -1): -0.81, (0, 0): 0.46, (0, 1): 0.25,
    (1, -1): -0.19, (1, 0): 0.93, (1, 1): -0.62,
}
BETA = sp.Symbol('beta')
_UPWIND = [(0, 0, 0), (0, 0, -1), (0, -1, 0), (-1, 0, 0)]


def _pick(box, keep):
    return {o: w for o, w in box.items() if keep(*o)}


# name -> {(dz, dy, dx): weight} on one field ``u``, one output ``out``
FAMILIES = {
    'shift': {(1, -1, 1): 1.0},                                            # a pure copy from one off-centre neighbour
    'no_zminus': _pick(BOX, lambda dz, dy, dx: dz >= 0),                   # 18 taps, nothing behind the centre plane
    'only_zplus': _pick(BOX, lambda dz, dy, dx: dz == 1),                  # 9 taps, all in plane z+1
    'plane_only': _pick(BOX, lambda dz, dy, dx: dz == 0),                  # 9 taps, a 2-D operator on a 3-D field
    'x_only': _pick(BOX, lambda dz, dy, dx: dz == 0 and dy == 0 and dx != 0),
    'no_dx': _pick(BOX, lambda dz, dy, dx: dx == 0),                       # 9 taps, no x neighbours
    'upwind': {o: BOX[o] for o in _UPWIND},                                # one-sided on every axis
    'no_centre': _pick(BOX, lambda dz, dy, dx: (dz, dy, dx) != (0, 0, 0)),  # 26 taps
    'q19': _pick(BOX, lambda dz, dy, dx: abs(dz) + abs(dy) + abs(dx) <= 2),  # the box without its corners
    'corners': _pick(BOX, lambda dz, dy, dx: dz and dy and dx),            # the 8 corners alone
    'symbol_weight': {**{o: BOX[o] for o in _UPWIND}, (0, 0, -1): BETA},   # ``upwind``, one weight passed at launch
}
# (dy, dx) tables for the 2-D views (``VIEW2D='yx'``: the field is one plane; ``'zy'``: its rows are the planes)
FAMILIES_2D = {
    'shift2': {(1, -1): 1.0},
    'x_only2': _pick(BOX2, lambda dy, dx: dy == 0 and dx != 0),
    'y_only2': _pick(BOX2, lambda dy, dx: dx == 0 and dy != 0),
    'no_centre2': _pick(BOX2, lambda dy, dx: (dy, dx) != (0, 0)),
    'corners2': _pick(BOX2, lambda dy, dx: dy and dx),
}
# two outputs whose tap sets touch different planes
TWO_SPARSE = {'o1': FAMILIES['only_zplus'], 'o2': FAMILIES['no_dx']}

NAMES_3D = tuple(FAMILIES) + ('two_sparse',)
NAMES_2D = tuple(FAMILIES_2D)
NONE_FAMILIES = ('shift', 'only_zplus', 'upwind', 'no_centre', 'two_sparse')    # where a wrong written box would differ
BETAS = (0.37, -0.81)                     # the two launch values of ``symbol_weight``


def outputs(name):
    """{output field name: tap table} of a family."""
    if name == 'two_sparse':
        return TWO_SPARSE
    return {'out': FAMILIES[name] if name in FAMILIES else FAMILIES_2D[name]}


def ndim(name):
    return 2 if name in FAMILIES_2D else 3


def scalars(name, value=BETAS[0]):
    """The launch-time scalars of a family ({} but for ``symbol_weight``)."""
    return {'beta': value} if name == 'symbol_weight' else {}


def numeric(taps, **values):
    """The tap table with its symbols replaced by ``values`` (by symbol name)."""
    return {o: float(w.subs({sp.Symbol(k): v for k, v in values.items()})) if isinstance(w, sp.Expr) else float(w)
            for o, w in taps.items()}


def collection(name, dtype='float32'):
    """The family as a ``ps.AssignmentCollection`` built through the public API."""
    from pystencils_autodiff_amd import ps
    outs = outputs(name)
    fields = ps.fields(f"u, {', '.join(outs)}: {dtype}[{ndim(name)}d]")
    u, by_name = fields[0], dict(zip(outs, fields[1:]))
    return ps.AssignmentCollection({by_name[n].center: sp.Add(*[(w if isinstance(w, sp.Expr) else sp.Float(w)) * u[o]
                                                                 for o, w in taps.items()])
                                    for n, taps in outs.items()})


def _shifted(a, off, bh):
    """``b[x] = a[x + off]``; cells read outside the domain are zeros, or wrap."""
    if bh == 'periodic':
        return np.roll(a, tuple(-o for o in off), axis=tuple(range(a.ndim)))
    assert bh == 'zeros', bh
    r = max([abs(o) for o in off] + [1])
    p = np.pad(a, r)
    return p[tuple(slice(r + o, r + o + n) for o, n in zip(off, a.shape))]


def plain_forward(taps, u, bh='zeros'):
    """``out[x] = Σ w · u[x + o]`` in float64."""
    u = np.asarray(u, dtype=np.float64)
    out = np.zeros_like(u)
    for off, w in taps.items():
        out += float(w) * _shifted(u, off, bh)
    return out


def plain_adjoint(taps, d, bh='zeros'):
    """``diffu[x] = Σ w · diffout[x − o]`` in float64: the transpose of ``plain_forward`` under the same ``bh``."""
    d = np.asarray(d, dtype=np.float64)
    out = np.zeros_like(d)
    for off, w in taps.items():
        out += float(w) * _shifted(d, tuple(-o for o in off), bh)
    return out


def reference(name, which, arrays, bh='zeros', absolute=False, **values):
    """{written field: float64 array} of a family's forward (``which='f'``, from ``u``) or adjoint (``'b'``, from the
    ``diff<output>`` arrays) sweep by the plain references; ``absolute``: Σ|w|·|input| per cell instead."""
    outs = {n: numeric(t, **values) for n, t in outputs(name).items()}
    if absolute:
        outs = {n: {o: abs(w) for o, w in t.items()} for n, t in outs.items()}
        arrays = {n: np.abs(np.asarray(a, dtype=np.float64)) for n, a in arrays.items()}
    if which == 'f':
        return {n: plain_forward(t, arrays['u'], bh) for n, t in outs.items()}
    return {'diffu': sum(plain_adjoint(t, arrays['diff' + n], bh) for n, t in outs.items())}


def n_terms(name, which):
    """Products summed per written cell."""
    outs = outputs(name)
    return max(len(t) for t in outs.values()) if which == 'f' else sum(len(t) for t in outs.values())

