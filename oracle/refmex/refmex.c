/* oracle/refmex/refmex.c -- the runtime behind oracle/refmex/mex.h (see there).  TEST INFRASTRUCTURE. */
#include "mex.h"
#include <stdarg.h>

static char   g_printed[1 << 16];
static size_t g_printed_len = 0;

size_t refmex_elem_size(mxClassID c) {
    switch (c) {
    case mxDOUBLE_CLASS: case mxINT64_CLASS: case mxUINT64_CLASS: return 8;
    case mxSINGLE_CLASS: case mxINT32_CLASS: case mxUINT32_CLASS: return 4;
    case mxINT16_CLASS: case mxUINT16_CLASS: case mxCHAR_CLASS:   return 2;
    case mxINT8_CLASS: case mxUINT8_CLASS: case mxLOGICAL_CLASS:  return 1;
    default: return 0;
    }
}

size_t refmex_numel(const mxArray* a) {
    size_t n = 1;
    for (mwSize i = 0; i < a->ndim; i++) n *= a->dims[i];
    return n;
}

static mxArray* new_array(mwSize ndim, const mwSize* dims, mxClassID c) {
    if (ndim > REFMEX_MAX_DIMS || refmex_elem_size(c) == 0) return NULL;
    mxArray* a = (mxArray*)calloc(1, sizeof(mxArray));
    if (!a) return NULL;
    a->ndim = ndim < 2 ? 2 : ndim;                       /* every MATLAB array has at least two dimensions */
    for (mwSize i = 0; i < a->ndim; i++) a->dims[i] = i < ndim ? dims[i] : 1;
    a->classid = c;
    return a;
}

mxArray* mxCreateNumericArray(mwSize ndim, const mwSize* dims, mxClassID c, mxComplexity flag) {
    if (flag != mxREAL) return NULL;
    mxArray* a = new_array(ndim, dims, c);
    if (!a) return NULL;
    size_t n = refmex_numel(a);
    a->data = calloc(n ? n : 1, refmex_elem_size(c));
    a->owns_data = 1;
    if (!a->data) { free(a); return NULL; }
    return a;
}

mxArray* refmex_wrap(mwSize ndim, const mwSize* dims, mxClassID c, void* data) {
    mxArray* a = new_array(ndim, dims, c);
    if (a) a->data = data;
    return a;
}

void refmex_destroy(mxArray* a) {
    if (!a) return;
    if (a->owns_data) free(a->data);
    free(a);
}

void*   mxGetData(const mxArray* a) { return a->data; }
double* mxGetPr(const mxArray* a) { return (double*)a->data; }
size_t  mxGetM(const mxArray* a) { return a->dims[0]; }

size_t mxGetN(const mxArray* a) {
    size_t n = 1;
    for (mwSize i = 1; i < a->ndim; i++) n *= a->dims[i];
    return n;
}

double mxGetScalar(const mxArray* a) {
    const void* p = a->data;
    switch (a->classid) {
    case mxDOUBLE_CLASS: return *(const double*)p;
    case mxSINGLE_CLASS: return *(const float*)p;
    case mxINT8_CLASS:   return *(const int8_t*)p;
    case mxUINT8_CLASS: case mxLOGICAL_CLASS: return *(const uint8_t*)p;
    case mxINT16_CLASS:  return *(const int16_t*)p;
    case mxUINT16_CLASS: case mxCHAR_CLASS: return *(const uint16_t*)p;
    case mxINT32_CLASS:  return *(const int32_t*)p;
    case mxUINT32_CLASS: return *(const uint32_t*)p;
    case mxINT64_CLASS:  return (double)*(const int64_t*)p;
    case mxUINT64_CLASS: return (double)*(const uint64_t*)p;
    default: return 0.0;
    }
}

void* mxMalloc(size_t n) { return malloc(n ? n : 1); }
void  mxFree(void* p) { free(p); }

int mexPrintf(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    size_t room = sizeof(g_printed) - g_printed_len;
    int n = vsnprintf(g_printed + g_printed_len, room, fmt, ap);
    va_end(ap);
    if (n > 0) g_printed_len += (size_t)n < room ? (size_t)n : room - 1;
    return n;
}

const char* refmex_printed(void) { return g_printed; }
void refmex_clear_printed(void) { g_printed_len = 0; g_printed[0] = 0; }
