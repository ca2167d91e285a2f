/* Stand-in for <sndfile.h>: the one call audiosink.cpp makes while dumping, which the golden
 * driver never starts.  Used only by tests/golden/make_sink_golden.py. */
#ifndef SINK_STUB_SNDFILE
#define SINK_STUB_SNDFILE
#include <stdint.h>
typedef int64_t sf_count_t;
typedef struct SNDFILE_tag SNDFILE;
sf_count_t sf_writef_float(SNDFILE *sndfile, const float *ptr, sf_count_t frames);
#endif
