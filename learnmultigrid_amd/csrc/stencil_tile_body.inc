// The body of stencil_tile_kernel (stencil_tile.hip), which includes this text twice inside the kernel: once with INT = true
// for a tile that lies inside the grid, once with INT = false for every other tile.  It is text and not a function or a
// lambda on purpose: behind one more level of captures the compiler no longer sees the kernel's argument block and its LDS
// arrays for what they are, and even the kernels that have no second body came out with some ten more VGPRs, SGPR
// spills and scratch (profiles/tile_interior_resources.txt).  Everything it names is declared in the kernel in front of
// the inclusion; `return` leaves the kernel.
    // (INT: in a scalar register, so that a line's base address and the tests on its number are scalar work)
    const int rb0 = INT ? __builtin_amdgcn_readfirstlane(wave * RB) : wave * RB;

    // ---- request: every global load of the prologue, from addresses that are valid whatever the element is ----------
    // (the rule and its reason: head of stencil_tile.hip)
    struct Raw {                                                  // one element of a wave line as it comes out of memory
        double x, b;
        int pid, ppid, rpid;
        d2u e01, e23;                                             // PROL: the 2 x 2 coarse window, two 16-byte loads
    };
    Raw raw[RB];
    bool ok[RB];
    // PROL: bit 0 / 1: the first / second load of the window starts where the window does, bit 2 / 3: parity of the
    // element's own line / column -- one register per line instead of the 64-bit indices they come from
    int wf[PROL ? RB : 1];
    bool crow[(REST && !HX) ? RB : 1];                            // REST: the element carries a row of R
    // REST with HX: this thread's coarse node -- line t >> 5, column t & 31 of the even nodes of the inner part
    int rq = 0, rrow = H, rcol = H;
    bool rown = false, rhas = false;
    // (INT: the node's offset from the tile's first node in the coarse vector; below 2^31 where the thread owns a node)
    auto rnode = [&]() -> unsigned { return (unsigned)(t >> 5) * (unsigned)a.Wc + (unsigned)(t & 31); };
    if (REST && HX) {
        const int ye0 = (y0 + H + 1) & ~1, xe0 = (c0 + H + 1) & ~1;   // (y0 + H, c0 + H >= 0)
        const int yf = ye0 + 2 * (t >> 5), xf = xe0 + 2 * (t & 31);
        rown = INT ? (yf < y0 + RR - H && xf < c0 + kCols - H)
                   : (yf < y0 + RR - H && yf < a.lines && xf < c0 + kCols - H && xf < W);
        const int64_t jc = (int64_t)(yf >> 1) * a.Wc + (xf >> 1);
        rhas = rown && (INT || jc < a.nc);
        if (INT)                                                  // scalar base (the tile's first node) + node offset
            rq = (int)(a.rpid + ((int64_t)(ye0 >> 1) * a.Wc + (xe0 >> 1)))[rown ? rnode() : 0u];
        else
            rq = (int)a.rpid[rhas ? jc : 0];
        rrow = rown ? yf - y0 : H;
        rcol = rown ? xf - c0 : H;
    }
    // PROL with HX: the usual pair of P as values in scalar registers (a select between two kernel arguments that the
    // compiler can still see as such becomes a load from the argument block, indexed by the lane: a round trip)
    int phot[2] = {-1, -1};
    double phv[9] = {};
    if (PROL && HX) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            phot[s] = a.phot[s];
            asm volatile("" : "+s"(phot[s]));
        }
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            phv[s] = a.phv[s];
            asm volatile("" : "+s"(phv[s]));
        }
    }
    auto request = [&](int k) {
        const int y = y0 + rb0 + k;
        if constexpr (INT) {
            // the line's base is a scalar, the lane the offset: no 64-bit index per element, nothing to clamp
            const int64_t i0 = (int64_t)y * W + c0;
            ok[k] = true;
            raw[k].x = ZERO ? 0.0 : (a.x + i0)[lane];
            raw[k].b = (a.b + i0)[lane];
            raw[k].pid = (int)(a.pid + i0)[lane];
            if (PROL) {
                // line parity from the scalar y, column parity from the lane and the parity of c0; both window loads
                // start where the window does
                const int64_t base = (int64_t)(y >> 1) * a.Wc + (c0 >> 1);
                const int xo = (lane + (c0 & 1)) >> 1;
                raw[k].ppid = (int)(a.ppid + i0)[lane];
                raw[k].e01 = *reinterpret_cast<const d2u *>(a.ec + base + xo);
                raw[k].e23 = *reinterpret_cast<const d2u *>(a.ec + (base + a.Wc) + xo);
                wf[k] = 3 | ((y & 1) << 2) | (((c0 + lane) & 1) << 3);
            }
            if (REST && !HX) {
                const int c = c0 + lane;
                crow[k] = !(y & 1) && !(c & 1);
                const int64_t jc = (int64_t)(y >> 1) * a.Wc + (c >> 1);
                raw[k].rpid = (int)a.rpid[(crow[k] && jc < a.nc) ? jc : 0];
            }
            return;
        }
        const int64_t i = (int64_t)y * W + c0 + lane;
        // (linear validity: an element outside the lines 0 .. lines - 1 whose index is a row -- (-1, W) is row 0, (lines, -1)
        // row n - 1 -- is that row, which operators with an entry across a line end read)
        ok[k] = i >= 0 && i < n;
        const int64_t j = ok[k] ? i : 0;
        raw[k].x = ZERO ? 0.0 : a.x[j];
        raw[k].b = a.b[j];
        raw[k].pid = (int)a.pid[j];
        if (PROL) {
            // the element is row j of P whatever its place in the tile (a column outside [0, W) is an element of the
            // adjacent line): its own line and column decide the window.  On grids at least two tiles wide one step to
            // the neighbouring line is enough; narrower ones divide.
            const int c = c0 + lane;
            int yy, xx;
            if (a.W >= 2 * kCols) {                               // uniform
                yy = c < 0 ? y - 1 : (c >= a.W ? y + 1 : y);
                xx = c < 0 ? c + a.W : (c >= a.W ? c - a.W : c);
            } else {
                yy = (int)((unsigned)j / (unsigned)a.W);
                xx = (int)((unsigned)j - (unsigned)yy * (unsigned)a.W);
            }
            const int64_t base = (int64_t)(yy >> 1) * a.Wc + (xx >> 1);
            raw[k].ppid = (int)a.ppid[j];
            // slots 0, 1 and 2, 3 are neighbours in memory: two 16-byte loads (8-byte aligned is enough); slots a
            // pattern does not have may point anywhere inside the vector
            const int64_t b0 = ok[k] ? min(base, (int64_t)a.nc - 2) : 0, b1 = ok[k] ? min(base + a.Wc, (int64_t)a.nc - 2) : 0;
            raw[k].e01 = *reinterpret_cast<const d2u *>(a.ec + b0);
            raw[k].e23 = *reinterpret_cast<const d2u *>(a.ec + b1);
            wf[k] = (b0 == base ? 1 : 0) | (b1 == base + a.Wc ? 2 : 0) | ((yy & 1) << 2) | ((xx & 1) << 3);
        }
        if (REST && !HX) {
            // elements on (even line, even column) of the grid carry a row of R
            const int c = c0 + lane;
            crow[k] = ok[k] && !(y & 1) && !(c & 1) && c >= 0 && c < W;
            const int64_t jc = (int64_t)(y >> 1) * a.Wc + (c >> 1);
            raw[k].rpid = (int)a.rpid[(crow[k] && jc < a.nc) ? jc : 0];
        }
    };
    // The loaded values pass through empty asm statements: a load cannot sink into a branch behind one, and no use can
    // rise above it.  The last request comes first, so that the one wait stands in front of it.
    auto arrived = [&](int k) {
        if (PROL && INT)                                          // (wf is two parity bits: nothing of it waits for a load)
            asm volatile("" : "+v"(raw[k].ppid), "+v"(raw[k].e01.a), "+v"(raw[k].e01.b), "+v"(raw[k].e23.a), "+v"(raw[k].e23.b));
        if (PROL && !INT)
            asm volatile("" : "+v"(raw[k].ppid), "+v"(raw[k].e01.a), "+v"(raw[k].e01.b), "+v"(raw[k].e23.a), "+v"(raw[k].e23.b),
                              "+v"(wf[k]));
        if (REST && !HX) asm volatile("" : "+v"(raw[k].rpid));
        if (!ZERO) asm volatile("" : "+v"(raw[k].x));
        asm volatile("" : "+v"(raw[k].b), "+v"(raw[k].pid));
    };
    // four lines with their windows in flight are 56 registers: those kernels ask for their lines one at a time
    constexpr int RG = (PROL && (RB > 2 || REST)) ? 1 : RB;
    static_assert(RB % RG == 0, "whole groups of lines");
#pragma unroll
    for (int k = 0; k < RG; ++k) request(k);
    // this thread's element of every table the workgroup stages (a block is at least as long as any table but the two
    // with nine values per pattern: their tail, if there is one, follows the consume step)
    static_assert(kBlock >= kMaxPat * 4, "one element of the short tables per thread");
    const int tv_n = a.npat * 9, tr_n = REST ? a.rp_npat * 9 : 1, tp_n = (PROL && !HX) ? a.pp_npat * 4 : 1;
    const int tm_i = min(t, a.npat - 1);
    double raw_sv = a.st_val[min(t, tv_n - 1)];                   // (staged in place: see lmg_common.hpp)
    int raw_sm = a.st_mask[tm_i];
    double raw_sd = a.st_val[tm_i * 9 + 4];                       // the diagonal: inside the table whatever the mask says
    double raw_rv = 0.0, raw_pv = 0.0;
    int raw_rm = 0, raw_pm = 0;
    if (REST) {
        raw_rv = a.rp_val[min(t, tr_n - 1)];
        raw_rm = a.rp_mask[min(t, a.rp_npat - 1)];
    }
    if (PROL && !HX) {
        raw_pv = a.pp_val[min(t, tp_n - 1)];
        raw_pm = a.pp_mask[min(t, a.pp_npat - 1)];
    }
    // (what needs no load goes here, behind the requests)
    for (int i = t; i < 2 * RR; i += kBlock) {                    // guard columns of both iterate buffers
        const int r = i >> 1, g = (i & 1) ? kLS - 1 : 0;
        s_x[0][r * kLS + g] = 0.0;
        s_x[1][r * kLS + g] = 0.0;
    }

    // ---- consume: nothing above this line uses a loaded value --------------------------------------------------------
    if (PROL && !HX) asm volatile("" : "+v"(raw_pv), "+v"(raw_pm));
    if (REST) asm volatile("" : "+v"(raw_rv), "+v"(raw_rm));
    asm volatile("" : "+v"(raw_sv), "+v"(raw_sm), "+v"(raw_sd));
#pragma unroll
    for (int k = RG - 1; k >= 0; --k) arrived(k);
    if (REST && HX) asm volatile("" : "+v"(rq));
    // (the tables' copies first: their registers are free before the lines need theirs; the reciprocals last, when the
    // lines' are free)
    if (t < tv_n) s_val[t] = raw_sv;
    if (REST) {
        if (t < tr_n) s_rv[t] = raw_rv;
        if (t < a.rp_npat) s_rm[t] = raw_rm;
    }
    if (PROL && !HX) {
        if (t < tp_n) s_pv[t] = raw_pv;
        if (t < a.pp_npat) s_pm[t] = raw_pm;
    }
    double lx[RB], bk[RB];
    int pk[RB];                                                   // pattern id | 0x100 where the element is a row of the matrix
    double le[(PROL && !HX) ? RB : 1][4];                         // PROL: the 2 x 2 coarse window of every element
    int lq[PROL ? RB : 1];                                        //       and its pattern id in P
    int lr[(REST && !HX) ? RB : 1];                               // REST: the id of R's row | 0x100 where the element has one
    if (REST && HX) rq = rhas ? (rq & 0xff) : 0;
    auto consume = [&](int k) {
        lx[k] = (!ZERO && ok[k]) ? raw[k].x : 0.0;
        bk[k] = ok[k] ? raw[k].b : 0.0;
        pk[k] = ok[k] ? ((raw[k].pid & 0xff) | 0x100) : 0;  // (& 0xff: behind the asm statement a byte is any int)
        if (PROL) {
            lq[k] = ok[k] ? (raw[k].ppid & 0xff) : 0;
            const d2u e01 = raw[k].e01, e23 = raw[k].e23;
            // (a window clamped at the end of the vector starts one element early: its first slot is the second value)
            const double w0 = (wf[k] & 1) ? e01.a : e01.b, w1 = e01.b, w2 = (wf[k] & 2) ? e23.a : e23.b, w3 = e23.b;
            if (!HX) {
                le[k][0] = w0;
                le[k][1] = w1;
                le[k][2] = w2;
                le[k][3] = w3;
            } else {
                // x + P e now: the sums of lmg_rpat_sweep_grid(SPMV, alpha = 1, beta = 1) in the same order
                const int yl = (wf[k] >> 2) & 1, xl = (wf[k] >> 3) & 1;
                // (read first, selected after: a select between two reads turns into one indexed read)
                const int h0 = phot[0], h1 = phot[1];
                const double p0 = phv[0], p1 = phv[1], p2 = phv[2], p3 = phv[3], p4 = phv[4], p5 = phv[5], p6 = phv[6], p7 = phv[7],
                             p8 = phv[8];
                const int hp = yl ? h1 : h0;
                const bool hotk = !ok[k] || (hp >= 0 && lq[k] == ((xl ? hp >> 8 : hp) & 0xff));
                double acc = 0.0;
                if (__all(hotk)) {                                // wave-uniform: the usual pair, slots 0 (1) (2) (3)
                    const double v0 = yl ? (xl ? p5 : p3) : (xl ? p1 : p0);
                    const double v1 = yl ? p6 : p2, v2 = xl ? p7 : p4;
                    acc = acc + v0 * w0;
                    double tv = acc + v1 * w1;
                    acc = xl ? tv : acc;
                    tv = acc + v2 * w2;
                    acc = yl ? tv : acc;
                    tv = acc + p8 * w3;
                    acc = (xl & yl) ? tv : acc;
                } else {
                    // (the one round trip left behind the wait: P's own row, which waves of the usual pair never ask for)
                    const int q = lq[k], m = a.pp_mask[q];
                    const double w[4] = {w0, w1, w2, w3};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const double tv = acc + a.pp_val[q * 4 + s] * w[s];
                        acc = ((m >> s) & 1) ? tv : acc;
                    }
                }
                lx[k] = (pk[k] >> 8) ? lx[k] + acc : 0.0;
            }
        }
        if (REST && !HX) lr[k] = crow[k] ? ((raw[k].rpid & 0xff) | 0x100) : 0;
    };
#pragma unroll
    for (int k = 0; k < RG; ++k) consume(k);
#pragma unroll
    for (int g = RG; g < RB; g += RG) {                           // (the remaining groups: a round trip each)
#pragma unroll
        for (int k = g; k < g + RG; ++k) request(k);
#pragma unroll
        for (int k = g + RG - 1; k >= g; --k) arrived(k);
#pragma unroll
        for (int k = g; k < g + RG; ++k) consume(k);
    }
    if (t < a.npat) {
        const int m = raw_sm;
        const double dg = (m & 16) ? raw_sd : 0.0;
        s_rdiag[t] = dg != 0.0 ? 1.0 / dg : 0.0;
        s_mask[t] = dg == 0.0 ? (m | (1 << 16)) : m;             // bit 16: no usable diagonal -> copy x
    }
    if constexpr (kBlock < kMaxPat * 9) {                         // more than kBlock / 9 patterns: the tails
        for (int i = t + kBlock; i < tv_n; i += kBlock) s_val[i] = a.st_val[i];
        if (REST)
            for (int i = t + kBlock; i < tr_n; i += kBlock) s_rv[i] = a.rp_val[i];
    }
    if (PROL && !HX) {
        __syncthreads();
        // x + P e: the sums of lmg_rpat_sweep_grid(SPMV, alpha = 1, beta = 1) in the same order
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int m = s_pm[lq[k]];
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double tv = acc + s_pv[lq[k] * 4 + q] * le[k][q];
                acc = ((m >> q) & 1) ? tv : acc;
            }
            lx[k] = (pk[k] >> 8) ? lx[k] + acc : 0.0;
        }
    }
    const int hot = a.hot >= 0 ? (a.hot | 0x100) : -1;
    bool mine = true;
#pragma unroll
    for (int k = 0; k < RB; ++k) {
        s_x[0][(rb0 + k) * kLS + 1 + lane] = lx[k];
        s_x[1][(rb0 + k) * kLS + 1 + lane] = 0.0;
        mine = mine && (pk[k] == hot || !(pk[k] >> 8));          // (elements outside the matrix are not stored)
    }
    // every lane of every line of this wave holds the frequent pattern: its values sit in scalar registers
    const bool all_hot = __all(mine);
    __syncthreads();

    const double omega = a.omega;
    double dk[CHEB ? RB : 1];                                     // CHEB: d of the lane's elements
    double hv[9];
#pragma unroll
    for (int s = 0; s < 9; ++s) hv[s] = a.hot_val[s];
    const double hrd = a.hot_rdiag;

    // A wave slides a three-line window down its lines: the centre values of a line come from LDS (one 8-byte read
    // per lane), its left / right neighbours from the neighbouring lanes (DPP; lanes 0 / 63 get the zero of the
    // guard columns -- they are halo), so a line costs one LDS read instead of nine.
    struct Win { double m, c, p; };
    auto line = [&](const double *src, int r, bool sides) -> Win {
        Win w;
        w.c = src[r * kLS + 1 + lane];
        if (LMG_TILE_LDS_SIDES) {
            // (the guard columns hold the zero that the DPP form fills in: the same bits, on the LDS pipe)
            w.m = sides ? src[r * kLS + lane] : 0.0;
            w.p = sides ? src[r * kLS + 2 + lane] : 0.0;
            return w;
        }
        w.m = sides ? dpp_lower<true>(w.c) : 0.0;
        w.p = sides ? dpp_upper<true>(w.c) : 0.0;
        return w;
    };
    // A x of the centre line of (u, c, d) for this lane, slot order = column order
    auto apply = [&](const Win &u, const Win &c, const Win &d, int p, bool hotp) -> double {
        const double w[9] = {u.m, u.c, u.p, c.m, c.c, c.p, d.m, d.c, d.p};
        double acc = 0.0;
        if (hotp) {
#pragma unroll
            for (int s = 0; s < 9; ++s)
                if ((UM >> s) & 1u) acc = acc + hv[s] * w[s];
        } else {
            const int q = p & 0xff, m = s_mask[q];
#pragma unroll
            for (int s = 0; s < 9; ++s) {
                if (!((UM >> s) & 1u)) continue;
                const double tv = acc + s_val[q * 9 + s] * w[s];
                acc = ((m >> s) & 1) ? tv : acc;
            }
        }
        return acc;
    };
    // The wave's block of RB lines, straight-line: all its lines are read first, then either the frequent pattern
    // everywhere or every line through the pattern table -- no branch inside either path, so the LDS latencies and
    // the dependent sums of the RB lines overlap.  Lines outside [lo, hi) are computed from clamped (meaningless)
    // neighbours and not kept.
    auto block = [&](const double *src, int lo, int hi, auto &&emit) {
        Win ln[RB + 2];
#pragma unroll
        for (int j = 0; j < RB + 2; ++j) {
            const int rr = min(max(rb0 - 1 + j, 0), RR - 1);
            ln[j] = line(src, rr, DIAG || (j >= 1 && j <= RB));
        }
        if (all_hot) {                                             // wave-uniform
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                const double acc = apply(ln[k], ln[k + 1], ln[k + 2], pk[k], true);
                emit(k, rb0 + k >= lo && rb0 + k < hi, true, ln[k + 1].c, acc);
            }
        } else {
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                const double acc = apply(ln[k], ln[k + 1], ln[k + 2], pk[k], false);
                emit(k, rb0 + k >= lo && rb0 + k < hi, false, ln[k + 1].c, acc);
            }
        }
    };

    // ---- the sweeps: iterate s goes from buffer (s - 1) & 1 to buffer s & 1 -------------------------------------
#pragma unroll
    for (int s = 1; s <= S; ++s) {
        const double *src = s_x[(s - 1) & 1];
        double *dst = s_x[s & 1];
        if (CHEB && ZERO && s == 1) {
            // first sweep from a zero iterate: x = d = c_0 * (D^-1 b)
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                dk[k] = a.chc[0] * (s_rdiag[pk[k] & 0xff] * bk[k]);
                dst[(rb0 + k) * kLS + 1 + lane] = (pk[k] >> 8) ? dk[k] : 0.0;
            }
        } else if (CHEB) {
            const double ca = a.cha[s - 1], cc = a.chc[s - 1];
            const bool first = s == 1;
            block(src, 1, RR - 1, [&](int k, bool keep, bool hotp, double xc, double acc) {
                const double res = bk[k] - acc;
                const int q = pk[k] & 0xff;
                const bool nodiag = !hotp && (s_mask[q] >> 16);
                const double z = (hotp ? hrd : s_rdiag[q]) * res;
                const double dn = first ? cc * z : ca * dk[k] + cc * z;
                dk[k] = nodiag ? 0.0 : dn;
                const double nx = nodiag ? xc : xc + dn;
                if (keep) dst[(rb0 + k) * kLS + 1 + lane] = (pk[k] >> 8) ? nx : 0.0;
            });
        } else if (ZERO && s == 1) {
            // first sweep from a zero iterate: x = omega * (D^-1 b) on every line (lmg_vmul's bits)
#pragma unroll
            for (int k = 0; k < RB; ++k)
                dst[(rb0 + k) * kLS + 1 + lane] = (pk[k] >> 8) ? omega * (s_rdiag[pk[k] & 0xff] * bk[k]) : 0.0;
        } else {
            // (lines 0 and RR - 1 have no line above / below)
            block(src, 1, RR - 1, [&](int k, bool keep, bool hotp, double xc, double acc) {
                const double res = bk[k] - acc;
                double nx;
                if (hotp) {
                    nx = xc + omega * (hrd * res);
                } else {
                    const int q = pk[k] & 0xff;
                    nx = (s_mask[q] >> 16) ? xc : xc + omega * (s_rdiag[q] * res);
                }
                if (keep) dst[(rb0 + k) * kLS + 1 + lane] = (pk[k] >> 8) ? nx : 0.0;
            });
        }
        __syncthreads();
    }

    // ---- outputs: the inner part of the tile, inside the line, rows of the matrix --------------------------------
    const double *fin = s_x[S & 1];
    const bool col_ok = lane >= H && lane < kCols - H && (INT || (c0 + lane >= 0 && c0 + lane < W));
    if (REST) {
        // the residual goes to the other LDS buffer (all lines but the first and the last: exact where it is read),
        // then every element that carries a row of R sums its nine entries in column order -- the sums of
        // lmg_rpat_sweep_grid(SPMV, alpha = 1, beta = 0)
        double *rl = s_x[(S + 1) & 1];
        block(fin, 1, RR - 1, [&](int k, bool keep, bool, double xc, double acc) {
            const int r = rb0 + k;
            if (keep) rl[r * kLS + 1 + lane] = bk[k] - acc;
            if (r >= H && r < RR - H && col_ok && (pk[k] >> 8)) a.out[(int64_t)(y0 + r) * W + c0 + lane] = xc;
        });
        __syncthreads();
        if (HX) {
            // a thread per coarse node; waves without one have nothing left to do
            if (__any(rown)) {
                const double *p = rl + rrow * kLS + 1 + rcol;
                double acc = 0.0;
                if (__all(!rown || rq == a.rhot)) {
#pragma unroll
                    for (int e = 0; e < 9; ++e) acc = acc + a.rhv[e] * p[(e / 3 - 1) * kLS + e % 3 - 1];
                } else {
                    const int m = s_rm[rq];
#pragma unroll
                    for (int e = 0; e < 9; ++e) {
                        const double tv = acc + s_rv[rq * 9 + e] * p[(e / 3 - 1) * kLS + e % 3 - 1];
                        acc = ((m >> e) & 1) ? tv : acc;
                    }
                }
                if (INT) {
                    const int ye0 = (y0 + H + 1) & ~1, xe0 = (c0 + H + 1) & ~1;
                    if (rown) (a.bc + ((int64_t)(ye0 >> 1) * a.Wc + (xe0 >> 1)))[rnode()] = acc;
                } else if (rown) {
                    a.bc[(int64_t)((y0 + rrow) >> 1) * a.Wc + ((c0 + rcol) >> 1)] = acc;
                }
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int r = rb0 + k;
            const int q = lr[k] & 0xff, m = s_rm[q];
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                const int rr = min(max(r + e / 3 - 1, 0), RR - 1);
                const double tv = acc + s_rv[q * 9 + e] * rl[rr * kLS + 1 + lane + e % 3 - 1];
                acc = ((m >> e) & 1) ? tv : acc;
            }
            if ((lr[k] >> 8) && r >= H && r < RR - H && col_ok)
                a.bc[(int64_t)((y0 + r) >> 1) * a.Wc + ((c0 + lane) >> 1)] = acc;
        }
    } else if (RESID) {
        block(fin, H, RR - H, [&](int k, bool keep, bool, double xc, double acc) {
            const int64_t i = (int64_t)(y0 + rb0 + k) * W + c0 + lane;
            if (keep && col_ok && (pk[k] >> 8)) {
                a.out[i] = xc;
                a.r[i] = bk[k] - acc;
            }
        });
    } else {
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int r = rb0 + k;
            if (r >= H && r < RR - H && col_ok && (pk[k] >> 8))
                a.out[(int64_t)(y0 + r) * W + c0 + lane] = fin[r * kLS + 1 + lane];
        }
    }
