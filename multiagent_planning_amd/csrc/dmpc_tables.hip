// dmpc_tables.hip -- the numbers every solve rests on (included by dmpc_api.hip behind dmpc_context.hip, whose upload_tables copies them to the
// device): the model matrices of the two extern "C" readers and build_tables, the per-case Gram and inverse-factor tables of dmpc_device.h.  Pure
// host arithmetic, partly in long double: no HIP call, no HIP type, so a plain C++ program can include it (tests/tables_main.cpp does, and
// tests/test_tables_cpu.py holds its output to recorded bits).  Of the context file it takes g_err alone, for the two readers' argument errors.

extern "C" int dmpc_model_matrices(const dmpc_params *prm, double *Lambda, double *Av, double *A0, double *Delta)
{
    if (!prm || prm->K < 1 || prm->K > 64) { g_err = "dmpc_model_matrices: bad params"; return -1; }
    const int Kh = prm->K, n = 3 * Kh;
    const double h = prm->h;
    // Same floating-point recurrences as the reference so the matrices agree bit for bit:
    //   row_k = Aux*row_{k-1} + [0 .. b .. 0]  (getPosMat.m:18-23, dmpc_soft_bound.m:100-105)
    //   A_init = Aux*A_init                     (dmpc_soft_bound.m:106-107)
    // with Aux = [I3 h*I3; 0 I3], b = [h^2/2*I3; h*I3].  Per axis the state is (pos,vel) so only the
    // two scalar sequences pr[j], vr[j] (coefficients of a_j) are needed.
    std::vector<double> pr(Kh, 0.0), vr(Kh, 0.0);
    double a0p = 1.0, a0v = 0.0;   // A_init(1,1), A_init(1,4) of the current power of Aux
    if (Lambda) memset(Lambda, 0, sizeof(double) * n * n);
    if (Av) memset(Av, 0, sizeof(double) * n * n);
    if (A0) memset(A0, 0, sizeof(double) * n * 6);
    for (int k = 0; k < Kh; ++k) {
        for (int j = 0; j < Kh; ++j) {
            const double np_ = 1.0 * pr[j] + h * vr[j];   // Aux rows 1:3
            const double nv_ = 1.0 * vr[j];               // Aux rows 4:6
            pr[j] = np_; vr[j] = nv_;
        }
        pr[k] += h * h / 2; vr[k] += h;
        a0v = 1.0 * a0v + h * 1.0;   // (Aux*A_init)(1,4) = A_init(1,4) + h*A_init(4,4)
        for (int j = 0; j < Kh; ++j)
            for (int a = 0; a < 3; ++a) {
                if (Lambda) Lambda[(size_t)(3 * k + a) * n + 3 * j + a] = pr[j];
                if (Av) Av[(size_t)(3 * k + a) * n + 3 * j + a] = vr[j];
            }
        if (A0)
            for (int a = 0; a < 3; ++a) { A0[(size_t)(3 * k + a) * 6 + a] = a0p; A0[(size_t)(3 * k + a) * 6 + 3 + a] = a0v; }
    }
    if (Delta) {   // getDeltaMat.m:2-8: [I 0 ..; -I I 0 ..; ...]
        memset(Delta, 0, sizeof(double) * n * n);
        for (int k = 0; k < Kh; ++k)
            for (int a = 0; a < 3; ++a) {
                Delta[(size_t)(3 * k + a) * n + 3 * k + a] = 1.0;
                if (k > 0) Delta[(size_t)(3 * k + a) * n + 3 * (k - 1) + a] = -1.0;
            }
    }
    return 0;
}

extern "C" int dmpc_posvel_matrix(double h, int Kh, double *Aaug)
{
    // getPosVelMat.m:24: Aaug = [new_row(K); [0 .. I3]; [I3 0 ..]]  (12 x 3K): final position and
    // velocity rows, then the selectors of the last and first acceleration
    if (!Aaug || Kh < 1) { g_err = "dmpc_posvel_matrix: bad arguments"; return -1; }
    const int n = 3 * Kh;
    memset(Aaug, 0, sizeof(double) * 12 * n);
    for (int j = 0; j < Kh; ++j)
        for (int a = 0; a < 3; ++a) {
            Aaug[(size_t)a * n + 3 * j + a] = h * h / 2 + (double)(Kh - 1 - j) * h * h;
            Aaug[(size_t)(3 + a) * n + 3 * j + a] = h;
        }
    for (int a = 0; a < 3; ++a) {
        Aaug[(size_t)(6 + a) * n + 3 * (Kh - 1) + a] = 1.0;
        Aaug[(size_t)(9 + a) * n + a] = 1.0;
    }
    return 0;
}

// Cholesky A = C C' of the K x K matrix a(i, j), C lower triangular.  The tables are held to their bits: the operations stay in this order
template <class Entry> static void cholesky_lower(Entry a, long double (&C)[K][K])
{
    memset(C, 0, sizeof(C));
    for (int j = 0; j < K; ++j) {
        long double d = a(j, j);
        for (int k = 0; k < j; ++k) d -= C[j][k] * C[j][k];
        C[j][j] = sqrtl(d);
        for (int i = j + 1; i < K; ++i) {
            long double t = a(i, j);
            for (int k = 0; k < j; ++k) t -= C[i][k] * C[j][k];
            C[i][j] = t / C[j][j];
        }
    }
}

// H1 = 2(q l_K l_K' + s D1'D1 + I)  (per-axis block of solveSoftDMPCbound.m:98); returns
// H1^-1, M1 = H1^-1 L', P1 = L H1^-1 L' (row-major 15x15 each)
static void build_case_tables(double h, double q, double s, double *out /*675*/, double *hsum = nullptr)
{
    long double L[K][K], H[K][K], Hi[K][K], C[K][K];
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) L[i][j] = (j <= i) ? ((long double)h * h / 2 + (long double)(i - j) * h * h) : 0.0L;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            long double dd = 0.0L;   // (D1'D1)_{ij}: tridiagonal [.. -1 2 -1 ..], last diagonal entry 1
            if (i == j) dd = (i == K - 1) ? 1.0L : 2.0L;
            else if (i == j + 1 || j == i + 1) dd = -1.0L;
            H[i][j] = 2.0L * ((long double)q * L[K - 1][i] * L[K - 1][j] + (long double)s * dd + (i == j ? 1.0L : 0.0L));
        }
    if (hsum) {   // sum of |H(i,j)|, rounded up: max over |a| <= alim of a'Ha/2 is at most alim^2/2 times this
        long double t = 0.0L;
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) t += fabsl(H[i][j]);
        *hsum = (double)(t * (1.0L + 1e-12L));
    }
    cholesky_lower([&](int i, int j) { return H[i][j]; }, C);
    // Hi = H^-1 column by column
    for (int c = 0; c < K; ++c) {
        long double y[K], x[K];
        for (int i = 0; i < K; ++i) {
            long double t = (i == c) ? 1.0L : 0.0L;
            for (int k = 0; k < i; ++k) t -= C[i][k] * y[k];
            y[i] = t / C[i][i];
        }
        for (int i = K - 1; i >= 0; --i) {
            long double t = y[i];
            for (int k = i + 1; k < K; ++k) t -= C[k][i] * x[k];
            x[i] = t / C[i][i];
        }
        for (int i = 0; i < K; ++i) Hi[i][c] = x[i];
    }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            long double sym = 0.5L * (Hi[i][j] + Hi[j][i]);
            out[i * K + j] = (double)sym;
        }
    long double M[K][K];
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            long double t = 0.0L;
            for (int k = 0; k < K; ++k) t += 0.5L * (Hi[i][k] + Hi[k][i]) * L[j][k];
            M[i][j] = t;
            out[225 + i * K + j] = (double)t;
        }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
            long double t = 0.0L;
            for (int k = 0; k < K; ++k) t += L[i][k] * M[k][j];
            out[450 + i * K + j] = (double)t;
        }
    // P1 is symmetric in exact arithmetic: symmetrise the rounded table
    for (int i = 0; i < K; ++i)
        for (int j = i + 1; j < K; ++j) {
            double m = 0.5 * (out[450 + i * K + j] + out[450 + j * K + i]);
            out[450 + i * K + j] = out[450 + j * K + i] = m;
        }
}

// the device tables: per cost case the symmetric 30x30 Gram table over (space, step) -- G[A i][A j] = H1^-1, G[A i][W j] =
// (H1^-1 L')(i,j), G[W i][W j] = L H1^-1 L' -- then Lt[k][kk] = Lambda(kk,k), then the inverse factors; hsum: see build_case_tables
static void build_tables(const dmpc_params &p, double *t /* TAB_ALL_DOUBLES */, double hsum[3])
{
    std::fill(t, t + TAB_ALL_DOUBLES, 0.0);
    const double sfree = p.Sfree > 0 ? p.Sfree : 10.0;
    const double qs[3] = {p.Qfar > 0 ? p.Qfar : 1000.0, p.Qnear > 0 ? p.Qnear : 10000.0, p.Q1};   // far (:44-47), near (:49-52), coll (:54-57)
    const double ss[3] = {sfree, sfree, (p.variant == DMPC_VAR_ALL3) ? 10.0 : p.S1};             // all:71
    for (int c = 0; c < 3; ++c) {
        double hmp[675];
        build_case_tables(p.h, qs[c], ss[c], hmp, &hsum[c]);
        double *G = &t[(size_t)c * TAB_CASE_DOUBLES];
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) {
                G[i * 30 + j] = hmp[i * K + j];
                G[i * 30 + 15 + j] = hmp[225 + i * K + j];
                G[(15 + j) * 30 + i] = hmp[225 + i * K + j];
                G[(15 + i) * 30 + 15 + j] = hmp[450 + i * K + j];
            }
        // Tp = C^-T with H1^-1 = C C' (the ROUNDED table above: the numbers the solver's Schur complement is made of).  The leading
        // m x m block of Tp is the inverse factor of the leading block of H1^-1: S^-1 = Tp Tp' for the bounds of steps 0..m-1 of one axis.
        // Second table: the same for the steps in FALLING order (14, 13, ..): H1^-1 with rows and columns reversed.
        for (int rev = 0; rev < 2; ++rev) {
            long double C[K][K], Ci[K][K];
            cholesky_lower([&](int i, int j) -> long double { return rev ? hmp[(K - 1 - i) * K + (K - 1 - j)] : hmp[i * K + j]; }, C);
            memset(Ci, 0, sizeof(Ci));
            for (int c2 = 0; c2 < K; ++c2)   // C^-1 column by column (forward substitution)
                for (int i = c2; i < K; ++i) {
                    long double v = (i == c2) ? 1.0L : 0.0L;
                    for (int k = c2; k < i; ++k) v -= C[i][k] * Ci[k][c2];
                    Ci[i][c2] = v / C[i][i];
                }
            double *Tp = &t[(size_t)TAB_DOUBLES + (size_t)(2 * c + rev) * TAB_TP_CASE];
            for (int i = 0; i < K; ++i)
                for (int j = i; j < K; ++j) Tp[i * (31 - i) / 2 + j - i] = (double)Ci[j][i];
        }
    }
    for (int k = 0; k < K; ++k)
        for (int kk = k; kk < K; ++kk) t[3 * TAB_CASE_DOUBLES + k * K + kk] = p.h * p.h / 2 + (double)(kk - k) * p.h * p.h;
}
