// calc_cost_sgm_linear MEX gateway -- drop-in for the reference's calc_cost_sgm.cpp built WITHOUT line 4 (#define USE_VZIND): the
// plain 1-D matcher along the per-pixel direction.
//   [bestD, minC, conf, bestD2] = calc_cost_sgm_linear(I1, I2, dMax, vMax, pixelPosD0, normlizeDirection,
//                                                      offsetFromPosD0, P1, P2)
// The nine arguments and four outputs of calc_cost_sgm; vMax and offsetFromPosD0 are read and checked like there and, as in that
// build of the reference, not used: candidate d lies d pixels along the direction (:368-369) and bestD is the index * 256.
// Environment: FSGM_DEVICE, FSGM_EPI_PATHS, FSGM_EPI_ADAPTIVE_P2 and FSGM_EPI_FB_CHECK as for calc_cost_sgm (the check works on
// bestD / 256, :453, :508).
// Everything computes on the GPU through libfsgm_hip.so; this file only unpacks mxArrays.
#include "gateway_common.h"

extern "C" void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    const char* fn = "calc_cost_sgm_linear";
    need_args(fn, nrhs, 9, nlhs, 4);
    size_t W = 0, H = 0;
    fsgm_epi_in in;
    in.I1 = need_u8_image(fn, prhs[0], "I1", &W, &H);                 // :548, :562-563
    in.I2 = need_u8_image(fn, prhs[1], "I2", &W, &H);
    in.width = (int32_t)W; in.height = (int32_t)H;
    in.dMax = need_int(fn, prhs[2], "dMax");                          // :551
    in.vMax = need_scalar(fn, prhs[3], "vMax");                       // :552 (unused in this build)
    in.pixelPosD0 = need_f64(fn, prhs[4], "pixelPosD0", W * H * 2);   // :553
    in.normDir = need_f64(fn, prhs[5], "normlizeDirection", W * H * 2);
    in.offset = need_f64(fn, prhs[6], "offsetFromPosD0", W * H);      // (unused in this build)
    in.P1 = need_int(fn, prhs[7], "P1");                              // :557-558
    in.P2 = need_int(fn, prhs[8], "P2");
    if (in.dMax < 1) mexErrMsgIdAndTxt("fsgm:range", "%s: dMax must be >= 1", fn);

    // outputs as the reference creates them (:569-572); conf and bestD2 stay zero unless FSGM_EPI_FB_CHECK=1
    Created made;
    mxArray* bestD = made.add(new_array(W, H, 1, mxUINT32_CLASS));
    mxArray* minC = made.add(new_array(W, H, 1, mxUINT32_CLASS));
    plhs[0] = bestD;
    if (nlhs > 1) plhs[1] = minC;
    if (nlhs > 2) plhs[2] = made.add(new_array(W, H, 1, mxUINT8_CLASS));
    if (nlhs > 3) plhs[3] = made.add(new_array(W, H, 1, mxUINT32_CLASS));

    fsgm_epi_out out;
    out.bestD = (uint32_t*)mxGetData(bestD);
    out.minC = (uint32_t*)mxGetData(minC);
    out.C = NULL; out.S = NULL;
    out.conf = nlhs > 2 ? (uint8_t*)mxGetData(plhs[2]) : NULL;
    out.bestD2 = nlhs > 3 ? (uint32_t*)mxGetData(plhs[3]) : NULL;
    fsgm_epi_params prm = fsgm_epi_params_default();
    prm.device = fsgm_env_int("FSGM_DEVICE", 0);
    prm.paths = fsgm_env_int("FSGM_EPI_PATHS", 4);
    prm.fb_check = fsgm_env_int("FSGM_EPI_FB_CHECK", 0) != 0;
    fsgm_epi_options opt = fsgm_epi_options_default();
    opt.adaptive_p2 = fsgm_env_int("FSGM_EPI_ADAPTIVE_P2", 0) != 0;
    fsgm_register_atexit();
    const fsgm_status st = fsgm_calc_cost_sgm_linear_host_opts(&in, &out, &prm, &opt);
    if (st != FSGM_OK) made.drop_all(nlhs, plhs);
    else if (nlhs <= 1) mxDestroyArray(minC);
    check_status(fn, st);
}
