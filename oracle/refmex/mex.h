/* oracle/refmex/mex.h -- a stand-in for MATLAB's mex.h, written from the public MEX API documentation.
 *
 * TEST INFRASTRUCTURE.  oracle/Makefile's `ref` target compiles the reference's four MEX sources, unmodified and from where
 * they lie, against this header and links them with refmex.c into oracle/_ref/ (git-ignored).  oracle/pyref.py then calls
 * their mexFunction with numpy buffers, so that the oracle and the kernels can be compared with what the reference's own code
 * computes.
 *
 * Why there are two headers: tests/mexstub/mex.h serves this project's own gateways (fsgm_amd/mex/) and is never used to build
 * anything from the reference tree; this one serves the reference's sources only and declares just what they use: mxGetData,
 * mxGetPr, mxGetScalar, mxGetM, mxGetN, mxCreateNumericArray, mxMalloc, mxFree, mxAssert, mexPrintf and the mexFunction
 * prototype, plus the <string.h> / <math.h> declarations that MATLAB's header brings in.
 */
#ifndef FSGM_REFMEX_MEX_H
#define FSGM_REFMEX_MEX_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef size_t mwSize;
typedef size_t mwIndex;

/* class ids as MATLAB's matrix.h numbers them */
typedef enum {
    mxUNKNOWN_CLASS = 0, mxCELL_CLASS, mxSTRUCT_CLASS, mxLOGICAL_CLASS, mxCHAR_CLASS, mxVOID_CLASS, mxDOUBLE_CLASS,
    mxSINGLE_CLASS, mxINT8_CLASS, mxUINT8_CLASS, mxINT16_CLASS, mxUINT16_CLASS, mxINT32_CLASS, mxUINT32_CLASS,
    mxINT64_CLASS, mxUINT64_CLASS
} mxClassID;

typedef enum { mxREAL = 0, mxCOMPLEX = 1 } mxComplexity;

#define REFMEX_MAX_DIMS 4

/* a plain real numeric array: dimensions, class, column-major data */
typedef struct mxArray_tag {
    mwSize    ndim;
    mwSize    dims[REFMEX_MAX_DIMS];
    mxClassID classid;
    void*     data;
    int       owns_data;          /* 1: data came from mxCreateNumericArray and goes with the array */
} mxArray;

mxArray* mxCreateNumericArray(mwSize ndim, const mwSize* dims, mxClassID classid, mxComplexity flag);   /* zero-filled */
void*    mxGetData(const mxArray* a);
double*  mxGetPr(const mxArray* a);
double   mxGetScalar(const mxArray* a);       /* first element, read by class, as a double */
size_t   mxGetM(const mxArray* a);            /* first dimension */
size_t   mxGetN(const mxArray* a);            /* product of dimensions 2 to the end, as MATLAB defines it */
void*    mxMalloc(size_t n);
void     mxFree(void* p);
int      mexPrintf(const char* fmt, ...);     /* appended to a capture buffer: refmex_printed() */

/* a release MEX build (no -g) compiles assertions out */
#define mxAssert(cond, msg) ((void)0)
#define mxAssertS(cond, msg) ((void)0)

/* the entry point every MEX file defines; C linkage, so the symbol is plain "mexFunction" */
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]);

/* ---- for the caller (oracle/pyref.py), not part of the MEX API ---- */
mxArray*    refmex_wrap(mwSize ndim, const mwSize* dims, mxClassID classid, void* data);   /* caller-owned buffer as an input */
void        refmex_destroy(mxArray* a);
size_t      refmex_numel(const mxArray* a);
size_t      refmex_elem_size(mxClassID classid);
const char* refmex_printed(void);
void        refmex_clear_printed(void);

#ifdef __cplusplus
}
#endif
#endif
