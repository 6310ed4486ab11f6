"""A plane step of the compute lanes (synchronise, the rows' taps, stores) and the plane loops around it."""
from ..hip_emitter import ws_plane_base
from .rows import row_prologue, taps
from .stores import stores


def step(T, k, ind, part='full', guard='jj < nplanes', store='jj >= 2'):
    """One plane with static set roles (k = plane index mod 3). ``part`` drops the taps of outputs outside the
    chunk: 'p0' = the chunk's first input plane (feeds output zb only), 'p1' = its second (not output zb-1),
    'e0' = the second to last (not output ze), 'e1' = the last (feeds output ze-1 only)."""
    cfg, NS = T.cfg, T.g['NS']
    sp, s0, sn = (k + 2) % 3, k, (k + 1) % 3
    sets = {'full': ((sp, 1), (s0, 0), (sn, -1)), 'p0': ((sn, -1),), 'p1': ((s0, 0), (sn, -1)),
            'e0': ((sp, 1), (s0, 0)), 'e1': ((sp, 1),)}[part]
    # the plane barrier as one asm statement with a memory clobber: the previous plane's LDS reads complete
    # (lgkmcnt) before it and none of them moves past it, none of this plane's moves above it (with
    # __syncthreads() hipcc 7.2 sank a peeled step's reads below the next step's barrier on the padded-row
    # image: the loader had already refilled that slot; scripts/probes/band_determinism.py)
    B = [f'{ind}if ({guard}) {{' if guard else f'{ind}{{']
    if T.free:
        # acquire: plane jj has landed once the loader's word exceeds jj (the last value seen is kept, so a wave
        # behind the loader polls no more); the memory clobbers keep this plane's LDS reads below the poll
        B += [f'{ind}  while ((int)seen <= jj) {{',
              f'{ind}    seen = __builtin_amdgcn_readfirstlane(hs_ld(0));',
              f'{ind}    if ((int)seen <= jj) __builtin_amdgcn_s_sleep(1);',
              f'{ind}  }}',
              f'{ind}  asm volatile("" ::: "memory");']
    else:
        B.append(f'{ind}  asm volatile("s_waitcnt lgkmcnt(0)\\n\\ts_barrier" ::: "memory");')
    B.append(f'{ind}  const {T.et}* sl = lds + (jj % {NS}) * {T.g["SLOT"]} + lofs;')
    if T.bo:
        # v_perm selectors: input row parity = plane parity ^ (y0 - 1 + row) & 1, y0 and R even -> odd rows r of
        # the lane take the plane's parity (selA), even rows the other one (selB); 0x05040302 = elements shifted
        # by one (the row was loaded one element early), 0x07060504 = the dword as it is
        B += [f'{ind}  const int ppq = hpar({ws_plane_base(T.S, 1, "(zb - 1 + jj)")});',
              # (scalar arithmetic, not selects: a select becomes a 64-bit lane mask per unrolled step)
              f'{ind}  const unsigned selA = 0x05040302u + (unsigned)ppq * 0x02020202u, '
              'selB = 0x07060504u - (unsigned)ppq * 0x02020202u;']
    # sets a trimmed step leaves alone are dead (outputs already stored or outside the chunk): overwrite them first
    # so their old values are not live through the step (a full step overwrites its q+1 set; +16-45 VGPRs else)
    for s_ in sorted({sp, s0, sn} - {st for st, _ in sets}):
        for si in range(T.NP):
            for o in range(T.R):
                B.append(f'{ind}  ' + ' '.join(f'{T.A(si, s_, o, a)} = {T.azero};' for a in range(4)))
    first = set()           # the (plan, row, slot) of set q+1 that took a dz = -1 tap this plane: filled by taps()
    for r in range(T.R + 2):
        B.append(f'{ind}  {{')
        B += row_prologue(T, ind, r)
        # every set every plane, one block: dx outer, then the three sets, rows and slots (12-36 independent
        # FMAs between two dependent ones)
        B += taps(T, f'{ind}    ', r, sets, first)
        B.append(f'{ind}  }}')
    if T.free:
        # release: this plane's LDS reads are complete; the loader may refill its slot
        B += [f'{ind}  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");',
              f'{ind}  if (lane == 0) hs_st(1 + wave, (unsigned)(jj + 1));',
              f'{ind}  asm volatile("" ::: "memory");']
    # outputs of q+1 that received no tap this plane (no dz = -1 taps) start from zero
    if any(dz == -1 for _, dz in sets):
        B += [f'{ind}  {T.A(si, sn, o, a)} = {T.azero};' for si in range(T.NP) for o in range(T.R) for a in range(4)
              if (si, o, a) not in first]
    if store is not None:
        # idle lanes (band tasks not a multiple of 64) compute on a clamped task with wrong x neighbours: no stores
        act = 'active' if T.g['ntask'] != T.g['NCT'] else ''
        cond = ' && '.join(c for c in (store, act) if c)
        if cfg.BABL == 2:
            cond = f'({cond}) && Z < 0' if cond else 'Z < 0'          # ablation probe: no output stores
        B.append(f'{ind}  if ({cond}) {{' if cond else f'{ind}  {{')
        for si, fld in enumerate(T.store_field):
            B += stores(T, f'{ind}    ', si, sp, fld)
        B.append(f'{ind}  }}')
    return B + [f'{ind}  ++jj;', f'{ind}}}']


def peeled_loop(T, ind, bound, guard, ends=False):
    """The chunk's first two input planes as peeled steps without the taps of outputs before it, then the loop of
    full steps at the roles (2, 0, 1) while ``jj < bound``, each under ``guard``. ``ends``: also the last two planes
    (the taps of outputs after the chunk), inside the loop at each static set role."""
    L = step(T, 0, ind, 'p0', None, None) + step(T, 1, ind, 'p1', None, None)
    if ends:
        L.append(f'{ind}const int nend = nplanes - 2;')
    L += [f'{ind}#pragma unroll 1', f'{ind}while (jj < {bound}) {{']
    for k in (2, 0, 1):
        L += step(T, k, f'{ind}  ', 'full', guard, '')
        for part, g in (('e0', 'jj == nend'), ('e1', 'jj < nplanes')) if ends else ():
            B = step(T, k, f'{ind}  ', part, g, '')
            L += [B[0].replace('if', 'else if', 1)] + B[1:]
    return L + [f'{ind}}}']


def plane_loops(T):
    """The lane's walk over the chunk's planes ``jj = 0 .. nplanes - 1`` by ``BTRIM``."""
    trim = T.cfg.BTRIM
    L = ['  unsigned seen = 0u;                               // planes known landed (hs[0])'] if T.free else []
    L.append('  int jj = 0;')
    if trim == 1:
        # the chunk's first two input planes run peeled steps without the taps of outputs before it (27 of 27·(zc+2)
        # FMAs per cell column); every chunk has >= 3 planes, so no fallback loop
        return L + peeled_loop(T, '  ', 'nplanes', 'jj < nplanes')
    if trim == 3:
        # chunks of exactly ZMIN planes (every chunk but a ragged last one): peeled first two planes, the main loop
        # over planes 2 .. ZMIN-1, the last two planes peeled after it at their static set roles (ZMIN is a compile-time
        # constant here); other chunks run the full loop
        zc = int(T.cfg.ZMIN)
        L.append(f'  if (nplanes == {zc + 2}) {{')
        L += peeled_loop(T, '    ', zc, f'jj < {zc}')
        k_end = zc % 3                     # set role of plane jj = zc (= nplanes - 2)
        L += step(T, k_end, '    ', 'e0', None, '') + step(T, (k_end + 1) % 3, '    ', 'e1', None, '')
        L.append('  } else {                         // a ragged chunk: peeled first two planes only (BTRIM=1)')
        return L + peeled_loop(T, '    ', 'nplanes', 'jj < nplanes') + ['  }']
    if trim == 2:
        # also the last two input planes (the taps of outputs after the chunk; 54 of 27·(zc+2) FMAs per cell
        # column), inside the unrolled loop at each static set role (a switch on jj % 3 after the loop made the
        # compiler select between the register sets: 192 VGPRs instead of 156); chunks of >= 3 planes
        L.append('  if (nplanes >= 5) {')
        L += peeled_loop(T, '    ', 'nplanes', 'jj < nend', ends=True)
        L.append('  } else {')
    L += ['  #pragma unroll 1', '  while (jj < nplanes) {']
    for k in range(3):
        L += step(T, k, '    ')
    return L + ['  }'] + (['  }'] if trim == 2 else [])
