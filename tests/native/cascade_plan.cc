// Prints what css_knn_plan.h decides, for tests/test_cascade_plan_host.py.  One answer line per request line on stdin:
//   plan <ntiles> <growth> <fill_stage0> <split_last>
//       -> "plan <n> <stride>,<ratio>,<count> ... | tickets <0|1> first <n + 1 ints> stride <n ints> gm1 <n ints>"
//   growth <kind> <i8> <k> <nrows> <env_growth> <env_growth_sweep>   -> "growth <g>"
//   eps <kind> <i8> <dpad>                                           -> "eps <bits of the float, hex>"
// kind: 0 batch, 1 VALU sweep, 2 int8-MFMA sweep.
#include "css_knn_plan.h"

#include <cstdio>
#include <cstring>

int main() {
    char line[256], what[16];
    while (fgets(line, sizeof line, stdin)) {
        long long a = 0, b = 0, c = 0, d = 0, e = 0, f = 0;
        if (sscanf(line, "%15s %lld %lld %lld %lld %lld %lld", what, &a, &b, &c, &d, &e, &f) < 1) continue;
        if (strcmp(what, "plan") == 0) {
            const CascadePlan p = cascade_plan(a, (int)b, c != 0, d != 0);
            printf("plan %d", p.n);
            for (int si = 0; si < p.n; ++si)
                printf(" %lld,%d,%lld", (long long)p.st[si].stride, p.st[si].ratio, (long long)p.st[si].count);
            int first[CZ_FS_MAXST + 1] = {}, stride[CZ_FS_MAXST] = {}, gm1[CZ_FS_MAXST] = {};
            const bool ok = cascade_tickets(p, (int)b, first, stride, gm1);
            printf(" | tickets %d", ok ? 1 : 0);
            if (ok) {
                printf(" first");
                for (int si = 0; si <= p.n; ++si) printf(" %d", first[si]);
                printf(" stride");
                for (int si = 0; si < p.n; ++si) printf(" %d", stride[si]);
                printf(" gm1");
                for (int si = 0; si < p.n; ++si) printf(" %d", gm1[si]);
            }
            printf("\n");
        } else if (strcmp(what, "growth") == 0) {
            printf("growth %d\n", cascade_growth((CascadeKind)a, b != 0, (int)c, d, (int)e, (int)f));
        } else if (strcmp(what, "eps") == 0) {
            const float v = cascade_eps_rel((CascadeKind)a, b != 0, (int)c);
            unsigned bits;
            memcpy(&bits, &v, 4);
            printf("eps %08x\n", bits);
        } else {
            printf("? %s\n", what);
        }
    }
    return 0;
}
