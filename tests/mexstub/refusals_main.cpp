// refusals_main.cpp -- a stand-alone host check of the two gateways that print a candidate count (calc_pyd_cost_sgm,
// calc_pyd_cost_sgm_ng): refused argument lists driven through mexFunction, built with -fsanitize=address,undefined by
// tests/test_mex_gateways_sanitizers.py.  A refusal happens before any call into libfsgm_hip.so, so the library's entry points
// are stand-ins here that fail the run when reached: the program links against the MEX stub alone, and no device is touched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>

#define mexFunction mex_calc_pyd_cost_sgm
#include "../../fsgm_amd/mex/calc_pyd_cost_sgm.cpp"
#undef mexFunction
#define mexFunction mex_calc_pyd_cost_sgm_ng
#include "../../fsgm_amd/mex/calc_pyd_cost_sgm_ng.cpp"
#undef mexFunction

static void reached(const char* what) { fprintf(stderr, "a refused call reached %s\n", what); exit(2); }
extern "C" {
const char* fsgm_last_error(void) { return ""; }
void fsgm_shutdown(void) {}
fsgm_status fsgm_calc_pyd_cost_sgm_host(const fsgm_pyd_in*, const fsgm_pyd_out*, int32_t) { reached("fsgm_calc_pyd_cost_sgm_host"); return FSGM_ERR_HIP; }
fsgm_status fsgm_calc_pyd_cost_sgm_ng_host(const fsgm_ng_in*, const fsgm_ng_out*, int32_t) { reached("fsgm_calc_pyd_cost_sgm_ng_host"); return FSGM_ERR_HIP; }
}

static const size_t W = 20, H = 12;
static int g_failed = 0;

static mxArray* image() {
    const mwSize d[2] = {W, H};
    mxArray* a = mxCreateNumericArray(2, d, mxUINT8_CLASS, mxREAL);
    for (size_t i = 0; i < W * H; i++) ((uint8_t*)mxGetData(a))[i] = (uint8_t)(i * 37u);
    return a;
}
static mxArray* hints() {
    const mwSize d[3] = {W, H, 2};
    return mxCreateNumericArray(3, d, mxDOUBLE_CLASS, mxREAL);
}

// one call with the given scalars after (I1, I2, preMv); it must be refused with `want` and leave nothing but its inputs
static void refused(const char* label, mexstub_fn fn, int nlhs, const std::vector<double>& scalars, const char* want) {
    const long before = mexstub_live_arrays();
    std::vector<const mxArray*> rhs = {image(), image(), hints()};
    for (double v : scalars) rhs.push_back(mxCreateDoubleScalar(v));
    mxArray* lhs[4] = {0, 0, 0, 0};
    const int rc = mexstub_call(fn, nlhs, lhs, (int)rhs.size(), rhs.data());
    const long leaked = mexstub_live_arrays() - before - (long)rhs.size();
    if (rc != 1 || strcmp(mexstub_last_error_id(), want) != 0 || leaked != 0) {
        fprintf(stderr, "%s: rc %d, identifier \"%s\" (wanted %s), %ld arrays left\n", label, rc, mexstub_last_error_id(), want, leaked);
        g_failed = 1;
    }
    for (const mxArray* a : rhs) mxDestroyArray((mxArray*)a);
}

int main() {
    const double big[] = {32, 1000, 23170, 46341, 1e6, 16};          // 2*23170+1 squared and 2*46341+1 squared leave int
    for (double h : big) {
        //            halfX halfY agg sub P1 P2 diag pass adaptive
        refused("pyd X=Y", mex_calc_pyd_cost_sgm, 3, {h, h, 2, 1, 6, 32, 1, 2, 0}, "fsgm:range");
        if (h > 31) refused("pyd X", mex_calc_pyd_cost_sgm, 3, {h, 0, 2, 1, 6, 32, 1, 2, 0}, "fsgm:range");
        if (h > 31) refused("pyd Y", mex_calc_pyd_cost_sgm, 3, {0, h, 2, 1, 6, 32, 1, 2, 0}, "fsgm:range");
    }
    const double ng_big[] = {4, 1000, 7736, 23170, 1e6, 2147483647.0, -1};   // 9 * (2*7736+1)^2 leaves int
    for (double h : ng_big) {
        //            half agg sub P1 P2
        refused("ng half", mex_calc_pyd_cost_sgm_ng, 2, {h, 2, 0, 6, 32}, "fsgm:range");
    }
    const double not_int[] = {NAN, INFINITY, -INFINITY, 2147483648.0, -2147483649.0, 1e300};
    for (double v : not_int) {
        refused("pyd P1", mex_calc_pyd_cost_sgm, 3, {2, 1, 2, 1, v, 32, 1, 2, 0}, "fsgm:range");
        refused("pyd totalPass", mex_calc_pyd_cost_sgm, 3, {2, 1, 2, 1, 6, 32, 1, v, 0}, "fsgm:range");
        refused("pyd halfX", mex_calc_pyd_cost_sgm, 3, {v, 1, 2, 1, 6, 32, 1, 2, 0}, "fsgm:range");
        refused("ng half", mex_calc_pyd_cost_sgm_ng, 2, {v, 2, 0, 6, 32}, "fsgm:range");
        refused("ng aggSize", mex_calc_pyd_cost_sgm_ng, 2, {1, v, 0, 6, 32}, "fsgm:range");
    }
    if (g_failed) return 1;
    printf("gateway refusals finished\n");
    return 0;
}
