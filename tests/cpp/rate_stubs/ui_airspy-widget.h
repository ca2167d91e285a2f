// TEST INFRASTRUCTURE: the widgets airspyHandler sets and never reads
#pragma once
#include <QFrame>
struct stubWidget {
    void setValue(int) {}
    void setText(const char *) {}
    void display(int) {}
};
class Ui_airspyWidget {
public:
    stubWidget w_;
    stubWidget *vgaSlider = &w_, *mixerSlider = &w_, *lnaSlider = &w_, *lnaButton = &w_, *mixerButton = &w_, *biasButton = &w_,
               *displaySerial = &w_, *lnaDisplay = &w_, *mixerDisplay = &w_, *vgaDisplay = &w_;
    void setupUi(QFrame *) {}
};
