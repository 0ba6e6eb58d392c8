// somar_amd/csrc/full19_point.inc -- the statements of full19_point.h's three functions, as text: one of them per inclusion,
// chosen by FULL19_PART.  full19_point.h includes it as the body of its functions; the k-marching kernels include it in place
// (see the header for why).  The including scope provides
//   Pn(di, dj, dk), En(di, dj, dk)   phi and the extrapolated copy at a constant offset from the cell (macros)
//   CF(n), SC(n)                     the cell's Full19Coef member n, the Full19Scales member n (macros)
//   alpha, beta                      the operator's coefficients
//   NEU(f)                           face f (xl, xh, yl, yh, zl, zh) is a Neumann domain face (part 3: is skipped)
//   FULL19_PART 1 (operator):  pc = phi of the cell;   result: double l
//   FULL19_PART 2 (interior):  rh = right-hand side; FULL19_LAPD, if defined, = lapDiag of the cell (else it is recomputed);
//                              result: F19_RESULT(value), a statement macro
//   FULL19_PART 3 (boundary):  rh;  result: F19_RESULT(value), a statement macro
#if FULL19_PART == 1
    // MAPPEDGETFLUX (beta = a_ref = 1) at the six faces: direction a, then b = a + 1, c = a + 2 (cyclic)
    double fxl = SC(a0) * CF(x0l) * (pc - Pn(-1, 0, 0)) +
                 SC(q1) * CF(x1l) * (En(0, 1, 0) - En(0, -1, 0) + En(-1, 1, 0) - En(-1, -1, 0)) +
                 SC(q2) * CF(x2l) * (En(0, 0, 1) - En(0, 0, -1) + En(-1, 0, 1) - En(-1, 0, -1));
    double fxh = SC(a0) * CF(x0h) * (Pn(1, 0, 0) - pc) +
                 SC(q1) * CF(x1h) * (En(1, 1, 0) - En(1, -1, 0) + En(0, 1, 0) - En(0, -1, 0)) +
                 SC(q2) * CF(x2h) * (En(1, 0, 1) - En(1, 0, -1) + En(0, 0, 1) - En(0, 0, -1));
    double fyl = SC(a1) * CF(y1l) * (pc - Pn(0, -1, 0)) +
                 SC(q2) * CF(y2l) * (En(0, 0, 1) - En(0, 0, -1) + En(0, -1, 1) - En(0, -1, -1)) +
                 SC(q0) * CF(y0l) * (En(1, 0, 0) - En(-1, 0, 0) + En(1, -1, 0) - En(-1, -1, 0));
    double fyh = SC(a1) * CF(y1h) * (Pn(0, 1, 0) - pc) +
                 SC(q2) * CF(y2h) * (En(0, 1, 1) - En(0, 1, -1) + En(0, 0, 1) - En(0, 0, -1)) +
                 SC(q0) * CF(y0h) * (En(1, 1, 0) - En(-1, 1, 0) + En(1, 0, 0) - En(-1, 0, 0));
    double fzl = SC(a2) * CF(z2l) * (pc - Pn(0, 0, -1)) +
                 SC(q0) * CF(z0l) * (En(1, 0, 0) - En(-1, 0, 0) + En(1, 0, -1) - En(-1, 0, -1)) +
                 SC(q1) * CF(z1l) * (En(0, 1, 0) - En(0, -1, 0) + En(0, 1, -1) - En(0, -1, -1));
    double fzh = SC(a2) * CF(z2h) * (Pn(0, 0, 1) - pc) +
                 SC(q0) * CF(z0h) * (En(1, 0, 1) - En(-1, 0, 1) + En(1, 0, 0) - En(-1, 0, 0)) +
                 SC(q1) * CF(z1h) * (En(0, 1, 1) - En(0, -1, 1) + En(0, 1, 0) - En(0, -1, 0));
    // EllipticConstNeumBCFluxClass: boundary faces := 0 (homogeneous)
    if (NEU(xl)) fxl = 0.0;
    if (NEU(xh)) fxh = 0.0;
    if (NEU(yl)) fyl = 0.0;
    if (NEU(yh)) fyh = 0.0;
    if (NEU(zl)) fzl = 0.0;
    if (NEU(zh)) fzh = 0.0;
    fxl *= beta; fxh *= beta; fyl *= beta; fyh *= beta; fzl *= beta; fzh *= beta;
    // MAPPEDFLUXDIVERGENCE3D, AXBYIP
    double l = CF(ji) * ((fxh - fxl) * SC(dxi0) + (fyh - fyl) * SC(dxi1) + (fzh - fzl) * SC(dxi2));
    if (alpha != 0.0) l = alpha * pc + 1.0 * l;
#elif FULL19_PART == 2
    // GSRBITER3D
    const double pdx = En(1, 0, 0) - En(-1, 0, 0);
    const double pdy = En(0, 1, 0) - En(0, -1, 0);
    const double pdz = En(0, 0, 1) - En(0, 0, -1);
    const double JDxx = CF(x0h) * Pn(1, 0, 0) + CF(x0l) * Pn(-1, 0, 0);
    const double JDxy = CF(x1h) * (En(1, 1, 0) - En(1, -1, 0) + pdy) - CF(x1l) * (pdy + En(-1, 1, 0) - En(-1, -1, 0));
    const double JDxz = CF(x2h) * (En(1, 0, 1) - En(1, 0, -1) + pdz) - CF(x2l) * (pdz + En(-1, 0, 1) - En(-1, 0, -1));
    const double JDyx = CF(y0h) * (En(1, 1, 0) - En(-1, 1, 0) + pdx) - CF(y0l) * (pdx + En(1, -1, 0) - En(-1, -1, 0));
    const double JDyy = CF(y1h) * Pn(0, 1, 0) + CF(y1l) * Pn(0, -1, 0);
    const double JDyz = CF(y2h) * (En(0, 1, 1) - En(0, 1, -1) + pdz) - CF(y2l) * (pdz + En(0, -1, 1) - En(0, -1, -1));
    const double JDzx = CF(z0h) * (En(1, 0, 1) - En(-1, 0, 1) + pdx) - CF(z0l) * (pdx + En(1, 0, -1) - En(-1, 0, -1));
    const double JDzy = CF(z1h) * (En(0, 1, 1) - En(0, -1, 1) + pdy) - CF(z1l) * (pdy + En(0, 1, -1) - En(0, -1, -1));
    const double JDzz = CF(z2h) * Pn(0, 0, 1) + CF(z2l) * Pn(0, 0, -1);
    const double lphi = beta * CF(ji) *
                        (JDxx * SC(xx) + JDyy * SC(yy) + JDzz * SC(zz) + (JDxy + JDyx) * SC(xy) +
                         (JDyz + JDzy) * SC(yz) + (JDzx + JDxz) * SC(zx));
#ifdef FULL19_LAPD
    const double lapd = FULL19_LAPD;   // the level's stored lapDiag
#else
    // lapDiag: FILLMAPPEDLAPDIAG3D's expression (k_lapdiag), bitwise the array launch_lapdiag fills
    const double lapd = -CF(ji) * ((CF(x0h) + CF(x0l)) * SC(xx) + (CF(y1h) + CF(y1l)) * SC(yy) + (CF(z2h) + CF(z2l)) * SC(zz));
#endif
    F19_RESULT((rh - lphi) / (alpha + beta * lapd));
#elif FULL19_PART == 3
    // GSRBBOUNDARYITER3D
    const bool sxl = NEU(xl), sxh = NEU(xh), syl = NEU(yl), syh = NEU(yh), szl = NEU(zl), szh = NEU(zh);
    double JDloX = 0, JDhiX = 0, JDloY = 0, JDhiY = 0, JDloZ = 0, JDhiZ = 0, ld = 0.0;
    if (!sxl) {
        JDloX = +SC(xx) * CF(x0l) * Pn(-1, 0, 0) -
                SC(xy) * CF(x1l) * (En(0, 1, 0) - En(0, -1, 0) + En(-1, 1, 0) - En(-1, -1, 0)) -
                SC(zx) * CF(x2l) * (En(0, 0, 1) - En(0, 0, -1) + En(-1, 0, 1) - En(-1, 0, -1));
        ld = ld - SC(xx) * CF(x0l);
    }
    if (!sxh) {
        JDhiX = +SC(xx) * CF(x0h) * Pn(1, 0, 0) +
                SC(xy) * CF(x1h) * (En(1, 1, 0) - En(1, -1, 0) + En(0, 1, 0) - En(0, -1, 0)) +
                SC(zx) * CF(x2h) * (En(1, 0, 1) - En(1, 0, -1) + En(0, 0, 1) - En(0, 0, -1));
        ld = ld - SC(xx) * CF(x0h);
    }
    if (!syl) {
        JDloY = -SC(xy) * CF(y0l) * (En(1, 0, 0) - En(-1, 0, 0) + En(1, -1, 0) - En(-1, -1, 0)) +
                SC(yy) * CF(y1l) * Pn(0, -1, 0) -
                SC(yz) * CF(y2l) * (En(0, 0, 1) - En(0, 0, -1) + En(0, -1, 1) - En(0, -1, -1));
        ld = ld - SC(yy) * CF(y1l);
    }
    if (!syh) {
        JDhiY = +SC(xy) * CF(y0h) * (En(1, 1, 0) - En(-1, 1, 0) + En(1, 0, 0) - En(-1, 0, 0)) +
                SC(yy) * CF(y1h) * Pn(0, 1, 0) +
                SC(yz) * CF(y2h) * (En(0, 1, 1) - En(0, 1, -1) + En(0, 0, 1) - En(0, 0, -1));
        ld = ld - SC(yy) * CF(y1h);
    }
    if (!szl) {
        JDloZ = -SC(zx) * CF(z0l) * (En(1, 0, 0) - En(-1, 0, 0) + En(1, 0, -1) - En(-1, 0, -1)) -
                SC(yz) * CF(z1l) * (En(0, 1, 0) - En(0, -1, 0) + En(0, 1, -1) - En(0, -1, -1)) +
                SC(zz) * CF(z2l) * Pn(0, 0, -1);
        ld = ld - SC(zz) * CF(z2l);
    }
    if (!szh) {
        JDhiZ = +SC(zx) * CF(z0h) * (En(1, 0, 1) - En(-1, 0, 1) + En(1, 0, 0) - En(-1, 0, 0)) +
                SC(yz) * CF(z1h) * (En(0, 1, 1) - En(0, -1, 1) + En(0, 1, 0) - En(0, -1, 0)) +
                SC(zz) * CF(z2h) * Pn(0, 0, 1);
        ld = ld - SC(zz) * CF(z2h);
    }
    ld = ld * CF(ji);
    const double lphi = beta * CF(ji) * (JDloX + JDhiX + JDloY + JDhiY + JDloZ + JDhiZ);
    F19_RESULT((rh - lphi) / (alpha + beta * ld));
#else
#error "FULL19_PART: 1 operator, 2 interior update, 3 boundary update"
#endif
#undef FULL19_PART
