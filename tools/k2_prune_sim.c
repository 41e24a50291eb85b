/* k2_prune_sim.c — development tool: how often K2's LPC jobs survive the
 * residual lower-bound pruning (flac_search16.hip residual_lb) on config-2
 * shaped frames, i.e. how many predictors per candidate pay for pass 2
 * (the exact bit count) and the partition search; and how many a bound
 * checked after 16, 32 or 48 of a lane's 64 samples would prune there
 * (what ending pass 1 early could save).  Jobs are simulated in
 * the kernel's order: FIXED always evaluated, LPC orders 12 .. 1, a job
 * pruned when its lane-sum bound exceeds (best finished LPC total - hdr).
 *
 * k2_prune_sim [frames] orders: instead, every order's bound and exact total
 * are formed first and the pruning is replayed with four job orders (12 .. 1
 * as the kernel; estimate_order's pick first; the true best first; ascending
 * lower bound) and with the threshold seeded by the VERBATIM size -- whether
 * another order or seed would leave fewer jobs for pass 2.
 *
 * Build: gcc -O2 -ffp-contract=off -o tools/bin/k2_prune_sim tools/k2_prune_sim.c -lm
 * (includes the CPU restatement oracle/flac_port.c for the LPC analysis).
 */
#include "../oracle/flac_port.c"

#include <stdio.h>

static uint64_t xs = 88172645463325252ull;
static double urand(void)
{
    xs ^= xs << 13;
    xs ^= xs >> 7;
    xs ^= xs << 17;
    return (double)(xs >> 11) / 9007199254740992.0;
}
static double grand(void)
{
    double u = urand() + 1e-300, v = urand();
    return sqrt(-2.0 * log(u)) * cos(2 * M_PI * v);
}

static float lb_lane(uint32_t lane_sum, uint32_t cnt)
{
    const float cf = (float)cnt;
    float U = 2.0f * (float)lane_sum - cf;
    U = U > 0.f ? U : 0.f;
    const float x = (U + cf) * 0.69314718f / cf;
    const float lb = x >= 1.0f ? cf * log2f(x) + cf * 1.44269504f : U + cf;
    const float l4 = lb - 4.0f;
    return l4 > 0.f ? (float)(uint32_t)l4 : 0.f;
}

/* jobs that reach pass 2 when the candidate's LPC jobs run in seq[] order
 * from a threshold seed (0xFFFFFFFF: none) */
static int replay(const int *seq, const uint32_t *lb, const uint32_t *hdr, const uint32_t *tot,
                  uint32_t seed)
{
    uint32_t best = seed;
    int survive = 0;
    for (int q = 0; q < 12; ++q) {
        const int o = seq[q];
        const uint32_t thr = best == 0xFFFFFFFFu ? 0xFFFFFFFFu : (best > hdr[o] ? best - hdr[o] : 0);
        if (thr != 0xFFFFFFFFu && lb[o] > thr)
            continue;
        survive++;
        if (tot[o] < best)
            best = tot[o];
    }
    return survive;
}

int main(int argc, char **argv)
{
    const int n_frames = argc > 1 ? atoi(argv[1]) : 400;
    const int orders_mode = argc > 2 && !strcmp(argv[2], "orders");
    long st_pass2[5] = {0}, best_is_12 = 0, n_white = 0;
    double lb_gap = 0, white_lb = 0, white_lb14 = 0, white_exact = 0;
    flacport_options o = {4096, 12, 0, 6, 1, 0, 1, 0, 0, 0, 0, 4096};
    enc_ctx *e = calloc(1, sizeof(enc_ctx));
    e->o = &o;
    e->qlp_precision = 12;
    e->max_rice = 14;
    e->win = calloc(4096, sizeof(double));
    e->xw = calloc(4096, sizeof(double));
    static int32_t L[4096], R[4096], C[4][4096], res[4096];
    long jobs = 0, pass2 = 0, subfr = 0;
    long per_order_pass2[13] = {0};
    long early[3] = {0, 0, 0}; double cost_all = 0, cost_saved[3] = {0, 0, 0};
    for (int f = 0; f < n_frames; ++f) {
        const double f1 = 100 + 1900 * urand(), f2 = 2000 + 10000 * urand();
        const double a1 = 0.05 + 0.55 * urand(), a2 = 0.3 * urand();
        const int white = urand() < 0.05;
        for (int i = 0; i < 4096; ++i) {
            const double ph = 2 * M_PI * (i + 4096.0 * f) / 44100.0;
            double l = (a1 * sin(ph * f1) + a2 * sin(ph * f2)) * 32767.0 + grand() * 64.0;
            double r = (a1 * sin(ph * f1 * 1.3) + a2 * sin(ph * f2 * 1.3)) * 32767.0 +
                       grand() * 64.0;
            if (white) {
                l = (urand() * 65536.0) - 32768.0;
                r = (urand() * 65536.0) - 32768.0;
            }
            l = round(l);
            r = round(r);
            L[i] = (int32_t)(l < -32768 ? -32768 : l > 32767 ? 32767 : l);
            R[i] = (int32_t)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
        }
        for (int i = 0; i < 4096; ++i) {
            C[0][i] = L[i];
            C[1][i] = R[i];
            C[2][i] = (L[i] + R[i]) >> 1;
            C[3][i] = L[i] - R[i];
        }
        for (int c = 0; c < 4; ++c) {
            const int32_t *s = C[c];
            const unsigned bps = c == 3 ? 17 : 16;
            /* LPC analysis as plan_lpc */
            double Rr[MAX_LPC + 1], lp[MAX_LPC][MAX_LPC], err[MAX_LPC];
            tukey_window(e, 4096);
            for (unsigned n = 0; n < 4096; n++)
                e->xw[n] = s[n] * e->win[n];
            for (unsigned lag = 0; lag <= 12; lag++) {
                double acc = 0.0;
                for (unsigned i = 0; i < 4096 - lag; i++)
                    acc += e->xw[i] * e->xw[i + lag];
                Rr[lag] = acc;
            }
            double k = Rr[1] / Rr[0];
            lp[0][0] = k;
            err[0] = Rr[0] * (1.0 - (k * k));
            for (unsigned i = 1; i < 12; i++) {
                double q = Rr[i + 1];
                for (unsigned j = 0; j < i; j++)
                    q -= (lp[i - 1][j] * Rr[i - j]);
                k = q / err[i - 1];
                for (unsigned j = 0; j < i; j++)
                    lp[i][j] = lp[i - 1][j] - (k * lp[i - 1][i - j - 1]);
                lp[i][i] = k;
                err[i] = err[i - 1] * (1.0 - (k * k));
            }
            uint32_t best = 0xFFFFFFFFu;
            subfr++;
            if (orders_mode) {
                uint32_t lbo[13], hdro[13], toto[13];
                int truebest = 12;
                for (int order = 12; order >= 1; --order) {
                    int32_t cq[MAX_LPC];
                    int sh;
                    quantize(lp[order - 1], order, 12, cq, &sh);
                    lpc_residual(s, 4096, order, cq, sh, res);
                    hdro[order] = 7 + 1 + order * bps + 9 + order * 12;
                    float lb = 0;
                    for (int lane = 0; lane < 64; ++lane) {
                        uint32_t sum = 0;
                        int a = lane * 64 - order, b = a + 64;
                        if (a < 0)
                            a = 0;
                        for (int i = a; i < b; ++i)
                            sum += (uint32_t)abs(res[i]);
                        lb += lb_lane(sum, lane ? 64 : 64 - order);
                    }
                    lbo[order] = (uint32_t)lb;
                    plan_residuals(e, res, 4096 - order, 4096, order, &e->cand_res);
                    toto[order] = hdro[order] + e->cand_res.bits;
                    lb_gap += 1.0 - (double)lbo[order] / e->cand_res.bits;
                    if (order == 12 || toto[order] <= toto[truebest]) /* ties: the lower order, as the encoder */
                        truebest = order;
                    if (white && order == 12) {
                        /* the bound with every lane's k capped at 14 */
                        double cap = 0;
                        for (int lane = 0; lane < 64; ++lane) {
                            uint64_t sum = 0;
                            int a = lane * 64 - order, b = a + 64;
                            if (a < 0)
                                a = 0;
                            for (int i = a; i < b; ++i)
                                sum += (uint32_t)abs(res[i]);
                            const double cnt = lane ? 64 : 64 - order, U = 2.0 * sum;
                            double m = 1e300;
                            for (int k = 0; k <= 14; ++k) {
                                const double v = cnt * k + U / (double)(1u << k);
                                m = v < m ? v : m;
                            }
                            cap += m;
                        }
                        n_white++;
                        white_lb += (double)(lbo[12] + hdro[12]) / (bps * 4096.0);
                        white_lb14 += (cap + hdro[12]) / (bps * 4096.0);
                        white_exact += (double)toto[12] / (bps * 4096.0);
                    }
                }
                best_is_12 += truebest == 12;
                int seq[4][12];
                const int est = (int)estimate_order(bps, 12, 12, 4096, err);
                for (int q = 0, a = 0, b = 0; q < 12; ++q) {
                    seq[0][q] = 12 - q;
                    if (q == 0) {
                        seq[1][a++] = est;
                        seq[2][b++] = truebest;
                    }
                    if (12 - q != est)
                        seq[1][a++] = 12 - q;
                    if (12 - q != truebest)
                        seq[2][b++] = 12 - q;
                    seq[3][q] = 12 - q;
                }
                for (int i = 1; i < 12; ++i) /* ascending lower bound + header */
                    for (int j = i; j > 0 && lbo[seq[3][j]] + hdro[seq[3][j]] <
                                                 lbo[seq[3][j - 1]] + hdro[seq[3][j - 1]]; --j) {
                        const int t = seq[3][j];
                        seq[3][j] = seq[3][j - 1];
                        seq[3][j - 1] = t;
                    }
                for (int q = 0; q < 4; ++q)
                    st_pass2[q] += replay(seq[q], lbo, hdro, toto, 0xFFFFFFFFu);
                st_pass2[4] += replay(seq[0], lbo, hdro, toto, bps * 4096u);
                jobs += 12;
                continue;
            }
            for (int order = 12; order >= 1; --order) {
                int32_t cq[MAX_LPC];
                int sh;
                quantize(lp[order - 1], order, 12, cq, &sh);
                lpc_residual(s, 4096, order, cq, sh, res);
                const uint32_t hdr = 7 + 1 + order * bps + 9 + order * 12;
                uint32_t thr = best == 0xFFFFFFFFu ? 0xFFFFFFFFu : (best > hdr ? best - hdr : 0);
                /* lane sums over the lane's 64 samples (lane 0 has 64 - order residuals) */
                float lb = 0;
                for (int lane = 0; lane < 64; ++lane) {
                    uint32_t sum = 0;
                    int a = lane * 64 - order, b = a + 64;
                    if (a < 0)
                        a = 0;
                    for (int i = a; i < b; ++i)
                        sum += (uint32_t)abs(res[i]);
                    lb += lb_lane(sum, lane ? 64 : 64 - order);
                }
                jobs++;
                {
                    const int D = order / 2 + 1;
                    const double cpl = (double)(D + 3) * 64; /* pass-1 VALU per lane-run */
                    cost_all += cpl;
                    const int cuts[3] = {16, 32, 48};
                    for (int q = 0; q < 3; ++q) {
                        float lbp = 0;
                        for (int lane = 0; lane < 64; ++lane) {
                            uint32_t sum = 0;
                            int a = lane * 64 - order, b = lane * 64 - order + cuts[q];
                            int cnt = cuts[q];
                            if (a < 0) { cnt += a; a = 0; }
                            for (int i = a; i < b; ++i)
                                sum += (uint32_t)abs(res[i]);
                            lbp += lb_lane(sum, cnt);
                        }
                        if (thr != 0xFFFFFFFFu && (uint32_t)lbp > thr) {
                            early[q]++;
                            cost_saved[q] += cpl * (64 - cuts[q]) / 64.0;
                        }
                    }
                }
                if (thr != 0xFFFFFFFFu && (uint32_t)lb > thr)
                    continue;
                pass2++;
                per_order_pass2[order]++;
                plan_residuals(e, res, 4096 - order, 4096, order, &e->cand_res);
                const uint32_t tot = hdr + e->cand_res.bits;
                if (tot < best)
                    best = tot;
            }
        }
    }
    if (orders_mode) {
        static const char *names[5] = {"order 12 .. 1 (the kernel's)", "estimate_order's pick first",
                                       "the true best first", "ascending lower bound",
                                       "12 .. 1, threshold seeded with VERBATIM"};
        printf("subframes %ld  LPC jobs %ld\n", subfr, jobs);
        for (int q = 0; q < 5; ++q)
            printf("%-40s pass2 %ld (%.2f per subframe)\n", names[q], st_pass2[q],
                   (double)st_pass2[q] / subfr);
        printf("true best order is 12 in %.1f %% of subframes\n", 100.0 * best_is_12 / subfr);
        printf("residual_lb below the exact residual bits by %.1f %% (mean over jobs)\n",
               100.0 * lb_gap / jobs);
        if (n_white)
            printf("white-noise subframes %ld, order 12: (bound + header) / VERBATIM %.3f, with k <= 14 "
                   "%.3f, exact / VERBATIM %.3f\n", n_white, white_lb / n_white, white_lb14 / n_white,
                   white_exact / n_white);
        return 0;
    }
    printf("subframes %ld  LPC jobs %ld  pass2 %ld (%.2f per subframe, %.1f %%)\n", subfr, jobs,
           pass2, (double)pass2 / subfr, 100.0 * pass2 / jobs);
    for (int q = 0; q < 3; ++q)
        printf("check after %d of 64: %.1f %% of jobs pruned there, pass-1 cost saved %.1f %%\n",
               16 * (q + 1), 100.0 * early[q] / jobs, 100.0 * cost_saved[q] / cost_all);
    for (int o2 = 12; o2 >= 1; --o2)
        printf("order %2d: pass2 in %.1f %% of subframes\n", o2, 100.0 * per_order_pass2[o2] / subfr);
    return 0;
}
