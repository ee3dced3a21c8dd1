// tdoa_ls_solve.inc -- the solve of k_ls and k_ls_stream (tdoa_ls.hip), as
// text: from the sub-sample lags tau[P] of row f, started at cells[f] (clamped
// to the grid), `iters` Levenberg-Marquardt steps, then the row's outputs.  It
// reads kp, cells, xy_ls, rms_out, iters, f, tau and the constants M, P of the
// including kernel.
    int cell = cells[f];
    cell = cell < 0 ? 0 : (cell >= kp.G ? kp.G - 1 : cell);
    const double sc = (double)kp.grid_scale;
    double u = (double)(cell % kp.grid_W - kp.half_w) / sc;
    double v = (double)(kp.half_h - cell / kp.grid_W) / sc;
    const double lu = (double)kp.half_w / sc, lv = (double)kp.half_h / sc;
    const double h = (double)kp.height, kf = (double)kp.fs / (double)kp.c;
    double ss = 0.0;
    for (int it = 0; it <= iters; it++) {
        const double n2 = u * u + v * v + h * h, n = sqrt(n2), n3 = n2 * n;
        const double k = h / n;
        const double px = k * u, py = k * v, pz = k * h;
        const double dxu = h * (1.0 / n - u * u / n3), dyu = h * (-v * u / n3),
                     dzu = h * (-h * u / n3);
        const double dxv = h * (-u * v / n3), dyv = h * (1.0 / n - v * v / n3),
                     dzv = h * (-h * v / n3);
        double d[M], du[M], dv[M];
#pragma unroll
        for (int m = 0; m < M; m++) {
            const double ex = px - (double)kp.mic_xy[2 * m], ey = py - (double)kp.mic_xy[2 * m + 1],
                         ez = pz;
            d[m] = sqrt(ex * ex + ey * ey + ez * ez);
            du[m] = (ex * dxu + ey * dyu + ez * dzu) / d[m];
            dv[m] = (ex * dxv + ey * dyv + ez * dzv) / d[m];
        }
        double a11 = 0.0, a12 = 0.0, a22 = 0.0, g1 = 0.0, g2 = 0.0;
        ss = 0.0;
        int p = 0;  // pairs (i, j), i < j, in the context's (lexicographic) order
#pragma unroll
        for (int i = 0; i < M; i++)
#pragma unroll
            for (int j = i + 1; j < M; j++, p++) {
                const double r = (d[j] - d[i]) * kf - tau[p];
                const double ju = (du[j] - du[i]) * kf, jv = (dv[j] - dv[i]) * kf;
                a11 += ju * ju;
                a12 += ju * jv;
                a22 += jv * jv;
                g1 += ju * r;
                g2 += jv * r;
                ss += r * r;
            }
        if (it == iters)
            break;
        const double lam = 1e-3 * (a11 + a22) + 1e-12;
        const double b11 = a11 + lam, b22 = a22 + lam;
        const double det = b11 * b22 - a12 * a12;
        u -= (b22 * g1 - a12 * g2) / det;
        v -= (b11 * g2 - a12 * g1) / det;
        u = u < -lu ? -lu : (u > lu ? lu : u);
        v = v < -lv ? -lv : (v > lv ? lv : v);
    }
    if (xy_ls) {
        xy_ls[2 * f] = (float)u;
        xy_ls[2 * f + 1] = (float)v;
    }
    if (rms_out)
        rms_out[f] = (float)sqrt(ss / (double)P);
