// Stand-in for the receiver's GUI class: the layer II decoder only keeps a pointer to it.
#ifndef MP2_STUB_GUI
#define MP2_STUB_GUI
class RadioInterface {};
#endif
