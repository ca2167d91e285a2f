// Stand-in for the receiver's GUI class: ip_dataHandler only connects its signals to it.
#ifndef IP_STUB_GUI
#define IP_STUB_GUI
class RadioInterface {};
#endif
