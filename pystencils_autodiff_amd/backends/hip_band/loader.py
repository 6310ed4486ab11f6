"""The loader wave of the band kernel: LDS-DMA plane loads into the slot ring, or the register-staged ``BREG`` path."""
from ..hip_emitter import halo_wait_lines, ws_plane_base


def hpar_lambda(ind):
    """``hpar``: the parity of a plane's first element (its pointer's bit 1), for rows on half dwords."""
    return f'{ind}auto hpar = [&](const void* b) {{ return (int)(((unsigned long long)b >> 1) & 1); }};   // 0 for nullptr'


def loader_wave(T):
    L = [f'  const int ldw = {T.NCW};', '  if (wave == ldw) {']
    L += reg_loader(T) if T.breg else dma_offsets(T) + dma_issue(T) + dma_loop(T)
    return L + ['    return;', '  }']


def dma_offsets(T):
    """``vo[i]``: the byte offset in its plane of the i-th 16-byte piece the lane loads (``vo1``: on odd planes)."""
    X, es, NPR, NPIECE = T.X, T.es, T.NPR, T.g['NPIECE']
    L = [f'    int vo[{T.g["NI"]}];']
    if T.bo:
        L += [f'    int vo1[{T.g["NI"]}];', hpar_lambda('    ')]
    L += ['    #pragma unroll', f'    for (int i = 0; i < {T.g["NI"]}; ++i) {{', '      const int k = i * 64 + lane;']
    if not T.bu and not T.padded:
        L.append(f'      vo[i] = k < {NPIECE} ? ((y0 - 1) * {X * es} + 16 * k) : 0x7ffffff0;   // row -1 / past Y: range '
                 'check')
        return L + ['    }']
    L.append(f'      const int rr = k / {NPR}, pc = k - rr * {NPR}, yy = y0 - 1 + rr;')
    if T.padded:
        # image row rr = one zero piece (out of range: the DMA writes zeros) + the row's pieces; one zero piece ends
        # the slot (the right neighbour of the last row's end)
        L.append(f'      vo[i] = (pc > 0 && rr < {T.TY + 2} && yy >= 0 && yy < Y) ? (yy * {X * es} + 16 * (pc - 1)) : '
                 '0x7ffffff0;')
    elif not T.bo:
        # rows of a pitch that is not a multiple of 16 bytes: each row's pieces start at the row (dword-aligned, the
        # LDS image keeps a 16-byte row pitch XP); the last piece runs past the row end (zero-filled below)
        L.append(f'      vo[i] = (k < {NPIECE} && yy >= 0 && yy < Y) ? (yy * {X * es} + 16 * pc) : 0x7ffffff0;')
    else:
        # rows on half dwords: a row starting on an odd element (plane parity pp of the plane's first element, the
        # row's own parity) is loaded from one element early; offsets from the plane's dword-aligned base, one set
        # per plane parity
        L += [f'      const bool ok = k < {NPIECE} && yy >= 0 && yy < Y;',
              f'      const int s0 = yy * {X} - (yy & 1), s1 = 1 + yy * {X} - ((yy & 1) ^ 1);   // even elements',
              '      vo[i] = ok ? 2 * s0 + 16 * pc : 0x7ffffff0;',
              '      vo1[i] = ok ? 2 * s1 + 16 * pc : 0x7ffffff0;']
    return L + ['    }']


def dma_issue(T):
    """``issue(q, slot)``: plane ``q`` into ring slot ``slot``, one LDS-DMA instruction per piece of the lane."""
    S, et = T.S, T.et
    L = ['    auto issue = [&](const int q, const int slot) {', f'      const {et}* pb = {ws_plane_base(S, 1, "q")};']
    if T.bo:
        L.append('      const int pp = hpar(pb);')
        L.append(f'      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(pb ? pb - pp : '
                 f'f_{S.name}), (short)0, pb ? (int)((YX * 2 + 2 * pp + 3) & ~3ll) : 0, 0x00020000);')
    else:
        L.append(f'      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(pb ? pb : '
                 f'f_{S.name}), (short)0, pb ? (int)(YX * {T.es}) : 0, 0x00020000);')
    L.append(f'      {et}* dst = lds + slot * {T.g["SLOT"]};')
    if T.cfg.BABL == 3:
        L.append('      if (Z < 0)   // ablation probe: no plane loads')
    L.append('      #pragma unroll')
    L.append(f'      for (int i = 0; i < {T.g["NI"]}; ++i)')
    L.append(f'        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + i * '
             f'{64 * T.VE}), 16, {"pp ? vo1[i] : vo[i]" if T.bo else "vo[i]"}, 0, 0, 0);')
    return L + ['    };']


def zero_fill(T):
    """Plane j has landed: zeros over the image columns past each row's end, which the row's last cells read as
    their right neighbours (nothing to fill on rows of whole pieces, or with ``BZF=0``)."""
    X, es, XP, et = T.X, T.es, T.XP, T.et
    NS, SLOT = T.g['NS'], T.g['SLOT']
    if not T.bu or T.czf:
        return []
    if T.bo:
        # zeros over the image columns past each row's last element (X + the row's parity .. XP)
        nz = XP - X
        L = [f'        const int ppj = hpar({ws_plane_base(T.S, 1, "(zb - 1 + j)")});',
             f'        {et}* img = lds + (j % {NS}) * {SLOT};',
             f'        for (int i = lane; i < {(T.TY + 2) * nz}; i += 64) {{',
             f'          const int rr = i / {nz}, c = i - rr * {nz}, pos = {X} + (ppj ^ ((y0 - 1 + rr) & 1)) + c;',
             f'          if (pos < {XP}) img[rr * {XP} + pos] = ({et})0;',
             '        }']
    else:
        # zeros over the image columns X .. XP of every row (the straddling last piece brought the next row's first
        # elements)
        ndw = (XP - X) * es // 4
        L = [f'        unsigned* img = (unsigned*)(lds + (j % {NS}) * {SLOT});',
             f'        for (int i = lane; i < {(T.TY + 2) * ndw}; i += 64) '
             f'img[(i / {ndw}) * {XP * es // 4} + {X * es // 4} + i % {ndw}] = 0u;']
    return ['      {'] + L + ['        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");', '      }']


def dma_loop(T):
    """``D`` planes ahead, then per plane: wait for its pieces, fill, publish (barrier or handshake word), refill."""
    D, NS, NI = T.D, T.g['NS'], T.g['NI']
    L = []
    if T.free:
        # slot reuse: plane p goes into the slot of plane p - NS, which every compute wave must have released
        # (hs[1 + w] >= p - NS + 1); one LDS dword per lane, a wave-wide vote, s_sleep between polls
        L += ['    auto wait_free = [&](const int need) {',
              '      if (need <= 0) return;',
              '      while (true) {',
              f'        const unsigned v = lane < {T.NCW} ? hs_ld(1 + lane) : 0xffffffffu;',
              '        if (__builtin_amdgcn_ballot_w64(v < (unsigned)need) == 0ull) break;',
              '        __builtin_amdgcn_s_sleep(1);',
              '      }',
              '      asm volatile("" ::: "memory");',
              '    };']
    if T.cfg.HWAIT:
        L += halo_wait_lines()
    L += [f'    for (int i = 0; i < {D}; ++i)',
          '      if (i < nplanes) issue(zb - 1 + i, i);',
          '    for (int j = 0; j < nplanes; ++j) {',
          '      // barrier j publishes plane j: the planes issued after it stay in flight',
          f'      const int after = min({D - 1}, nplanes - 1 - j);',
          '      switch (after) {']
    L += [f'        case {a}: asm volatile("s_waitcnt vmcnt({a * NI})" ::: "memory"); break;' for a in range(D)]
    L.append('      }')
    L += zero_fill(T)
    if T.free:
        # publish plane j (its DMA landed: the vmcnt wait above; the zero fill: its lgkmcnt wait), then refill
        L.append('      if (lane == 0) hs_st(0, (unsigned)(j + 1));')
        L.append(f'      if (j + {D} < nplanes) {{ wait_free(j + {D} - {NS} + 1); issue(zb - 1 + j + {D}, (j + {D}) % {NS}); }}')
    else:
        L.append('      __builtin_amdgcn_s_barrier();')
        L.append(f'      if (j + {D} < nplanes) issue(zb - 1 + j + {D}, (j + {D}) % {NS});')
    return L + ['    }']


def _reg_load(T, q):
    """Plane ``q``'s pieces into the registers ``ra`` (``ea``: the dword after a piece, for half-dword rows)."""
    B = ['    {',
         f'      const {T.et}* pb = {ws_plane_base(T.S, 1, "(" + q + ")")};',
         '      aa = pb ? (int)((unsigned long long)pb & 3ull) : 0;',
         '      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(pb ? '
         f'(const char*)pb - aa : (const char*)f_{T.S.name}), (short)0, pb ? (int)((aa + YX * {T.es} + 3) '
         '& ~3ll) : 0, 0x00020000);',
         '      #pragma unroll',
         f'      for (int i = 0; i < {T.g["NI"]}; ++i) {{',
         '        const int o = ((okm >> i) & 1u) ? ((aa + go[i]) & ~3) : 0x7ffffff0;',
         '        ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);']
    if T.half:
        B.append('        ea[i] = __builtin_amdgcn_raw_buffer_load_b32(rs, o + 16, 0, 0);')
    return B + ['      }', '    }']


def _reg_store(T, slot):
    """The registers' pieces realigned, their cells past X zeroed, into image slot ``slot``."""
    per = 4 // T.es
    kx = T.X % T.VE                                  # valid cells of a row's last piece
    # per dword of the last piece: mask of the bits kept
    keep = [0xffffffff if d * per + per - 1 < kx else 0x0000ffff if d * per < kx else 0 for d in range(4)]
    B = ['    {',
         f'      {T.et}* img = lds + {slot} * {T.g["SLOT"]};',
         '      #pragma unroll',
         f'      for (int i = 0; i < {T.g["NI"]}; ++i) {{',
         '        u32x4 v = ra[i];']
    if T.half:
        B += ['        if ((aa + go[i]) & 2) {            // the piece starts on a half dword',
              '          v = (u32x4){__builtin_amdgcn_alignbyte(v.y, v.x, 2u), __builtin_amdgcn_alignbyte(v.z, v.y, 2u), '
              '__builtin_amdgcn_alignbyte(v.w, v.z, 2u), __builtin_amdgcn_alignbyte(ea[i], v.w, 2u)};',
              '        }']
    return B + ['        if ((lastm >> i) & 1u) {                // cells past X: zeros (right neighbour of cell X-1)',
                '          ' + ' '.join(f'v.{"xyzw"[d]} &= {keep[d]:#x}u;' for d in range(4) if keep[d] != 0xffffffff),
                '        }',
                f'        *(u32x4*)(img + (i * 64 + lane) * {T.VE}) = v;',
                '      }',
                '    }']


def reg_loader(T):
    """Register-staged loader for rows whose pitch is not a multiple of 16 bytes: each lane owns 16-byte image pieces
    (pads, rows outside the plane: zeros); a row piece is read with 16-byte (and, on half-dword rows, one more 4-byte)
    buffer loads at the dword at or below it, realigned by v_alignbyte, its cells past X zeroed, and written to the
    padded image with ds_write_b128 -- aligned image, no zero fill, no DMA at a row's misaligned start."""
    X, VE, NPR, NI = T.X, T.VE, T.NPR, T.g['NI']
    L = [f'    int go[{NI}];                        // byte offset of the piece in its plane (row piece)',
         '    unsigned okm = 0u, lastm = 0u;       // pieces that are row data / a row\'s partial last piece',
         '    #pragma unroll',
         f'    for (int i = 0; i < {NI}; ++i) {{',
         '      const int k = i * 64 + lane;',
         f'      const int rr = k / {NPR}, pc = k - rr * {NPR}, yy = y0 - 1 + rr;',
         f'      const bool ok = pc > 0 && rr < {T.TY + 2} && yy >= 0 && yy < Y;',
         f'      go[i] = ok ? (yy * {X} + (pc - 1) * {VE}) * {T.es} : 0;',
         '      okm |= ok ? (1u << i) : 0u;',
         f'      lastm |= (ok && pc == {T.g["CPR"]}) ? (1u << i) : 0u;',
         '    }',
         f'    u32x4 ra[{NI}];']
    if T.half:
        L.append(f'    unsigned ea[{NI}];')
    L.append('    int aa = 0;')
    # planes 0 and 1 before the first barrier, then plane j+2 between barriers j and j+1 (loads, wait, writes:
    # the load latency is the loader's alone, hidden behind the compute of plane j; three slots: slot (j+2) % 3
    # held plane j-1, which every compute wave finished before barrier j). No registers live across a barrier
    # or the loop's back edge, so the compiler's own vmcnt waits are exact.
    L += _reg_load(T, 'zb - 1') + _reg_store(T, '0')
    L.append('    if (nplanes > 1) {')
    L += _reg_load(T, 'zb') + _reg_store(T, '1')
    L += ['    }',
          '    for (int j = 0; j < nplanes; ++j) {',
          '      asm volatile("s_waitcnt lgkmcnt(0)\\n\\ts_barrier" ::: "memory");',
          '      if (j + 2 < nplanes) {']
    L += _reg_load(T, '(zb + 1 + j)') + _reg_store(T, f'((j + 2) % {T.g["NS"]})')
    return L + ['      }', '    }']
