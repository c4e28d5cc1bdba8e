/*
 * ccsc_localcn_mex.c -- MEX gateway to libccsc's local contrast normalisation
 * (ccsc_local_cn, include/ccsc.h): the 'local_cn' branch of
 * image_helpers/CreateImages.m:299-369 followed by ZERO_MEAN (:652-657), per image,
 * for images and frames of any size H, W >= 7.
 * NOT compiled in this repository (no MATLAB / mex.h here); build on a MATLAB host with:
 *   mex -R2018a ccsc_localcn_mex.c -I../include -L../ccsc_code_iccv2017_amd -lccsc
 *
 *   out = ccsc_localcn_mex(I, devices)
 * I: real double [H, W] or [H, W, n] (further dimensions count as images); devices: GPU
 * indices as ccsc_device.m returns them, of which the first is used.  out: double of
 * size(I) holding single-precision values (local_cn.m casts it to single).  Only
 * doubles are marshalled.
 */
#include "mex.h"
#include "ccsc.h"

static ccsc_ctx* g_ctx = NULL;
static int32_t g_dev = -1;

static void cleanup(void) {
  if (g_ctx) ccsc_destroy(g_ctx);
  g_ctx = NULL;
  g_dev = -1;
}

/* the cached context when it serves the same device, else a new one */
static ccsc_ctx* context_for(const mxArray* a, char* err, size_t errlen) {
  if (!mxIsDouble(a) || mxGetNumberOfElements(a) < 1)
    mexErrMsgIdAndTxt("ccsc:devices", "devices must list at least one GPU index (double)");
  int32_t dev = (int32_t)mxGetDoubles(a)[0];
  if (g_ctx && g_dev == dev) return g_ctx;
  cleanup();
  g_ctx = ccsc_create_multi(&dev, 1, err, errlen);
  if (!g_ctx) mexErrMsgIdAndTxt("ccsc:hip", "%s", err);
  g_dev = dev;
  mexAtExit(cleanup);
  return g_ctx;
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  char err[1024] = {0};
  if (nrhs != 2) mexErrMsgIdAndTxt("ccsc:args", "ccsc_localcn_mex needs 2 arguments: I, devices");
  if (nlhs > 1) mexErrMsgIdAndTxt("ccsc:args", "ccsc_localcn_mex has one output");
  const mxArray* I = prhs[0];
  if (!mxIsDouble(I) || mxIsComplex(I)) mexErrMsgIdAndTxt("ccsc:I", "I must be real double");
  const mwSize nd = mxGetNumberOfDimensions(I);
  const mwSize* d = mxGetDimensions(I);
  if (nd < 2 || d[0] > 0x7fffffff || d[1] > 0x7fffffff)
    mexErrMsgIdAndTxt("ccsc:I", "I must be [H, W] or [H, W, n]");
  int64_t n = 1;
  for (mwSize i = 2; i < nd; ++i) n *= (int64_t)d[i];
  plhs[0] = mxCreateNumericArray(nd, d, mxDOUBLE_CLASS, mxREAL);
  if (mxIsEmpty(I)) return;
  ccsc_ctx* ctx = context_for(prhs[1], err, sizeof err);
  const int32_t rc = ccsc_local_cn(ctx, mxGetDoubles(I), mxGetDoubles(plhs[0]), n, (int32_t)d[0],
                                   (int32_t)d[1], err, sizeof err);
  if (rc) mexErrMsgIdAndTxt("ccsc:local_cn", "%s (code %d)", err, rc);
}
