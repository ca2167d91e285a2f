// Stand-in for the reference's msc-handler.h: fib-processor.h needs only what it includes, the
// reference's own dab-constants.h (audiodata, packetdata, the getBits family).  The generator
// includes this file first and defines the real header's include guard (MSC_DECODER), because
// fib-processor.h finds that header beside itself before any include path is searched.
#ifndef FIB_STUB_MSC_HANDLER
#define FIB_STUB_MSC_HANDLER
#include "dab-constants.h"
#endif
