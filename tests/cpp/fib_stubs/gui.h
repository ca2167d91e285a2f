// Stand-in for the reference's gui.h: fib_processor only connects its signals to a RadioInterface.
#ifndef FIB_STUB_GUI
#define FIB_STUB_GUI
#include "QObject"
class RadioInterface : public QObject {};
#endif
